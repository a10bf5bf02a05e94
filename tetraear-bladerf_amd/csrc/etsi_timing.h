// etsi_timing.h -- the ETSI timing stage's device code, inlined by k_timing (etsi_timing.hip) and by
// the fused channel filters (etsi_chanfilt.hip, etsi_chanfilt_r.hip, through etsi_chanfilt.h's
// timing_tail): the wave butterflies, the interpolator, the Oerder-Meyr sums, the Gardner tracking
// loop with its CFO sums (timing_track, cfo_consumer) and the decision pass.  It restates
// oracle/etsi_oracle.c operation for operation (explicit fmaf, emulated 64-lane reductions, a
// libm-free atan2), so GPU and oracle results are bit-identical.  All of it device-only and
// __forceinline__; at the end, the declarations of what etsi_timing.hip gives the host chain.
#pragma once
#include <cfloat>

#include "common.h"

namespace {

// --------------------------------------------------------------------------- E2 timing
// 64-lane xor butterfly, levels 32, 16, .., LO: v_l + v_{l ^ off} at each level (the oracle's
// tree; fp add is commutative, so operand order within a pair is free).  Cross-lane moves stay in
// the VALU: permlane32/16 swaps for 32 and 16, DPP row rotations / quad permutes below (after the
// xor-8 level a lane's value depends only on l mod 8, so rotating a row by 4 reads l ^ 4's value,
// and by the same argument quad_perm covers 2 and 1) -- a ds_bpermute per level would put an LDS
// round trip on the Gardner loop's critical path.
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
    // bound_ctrl: a lane without a source reads 0 (only wave_shr's lane 0, which is replaced);
    // this form folds into the consuming v_add_f32_dpp
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int LO>
__device__ __forceinline__ float bfly(float v) {
    const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(b[0]) + __uint_as_float(b[1]);
    if constexpr (LO <= 8) v = v + dppf<0x128>(v);   // row_ror:8
    if constexpr (LO <= 4) v = v + dppf<0x124>(v);   // row_ror:4
    if constexpr (LO <= 2) v = v + dppf<0x4E>(v);    // quad_perm [2,3,0,1]
    if constexpr (LO <= 1) v = v + dppf<0xB1>(v);    // quad_perm [1,0,3,2]
    return v;
}
__device__ __forceinline__ float wave_sum(float v) { return bfly<1>(v); }
// two full butterflies level by level, interleaved: the Gardner block's error and power sums are
// one dependent chain each, and issued one after the other they doubled the loop's reduction latency
__device__ __forceinline__ void wave_sum2(float &u, float &v) {
    const auto a0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(u), __float_as_uint(u), false, false);
    const auto a1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    u = __uint_as_float(a0[0]) + __uint_as_float(a0[1]);
    v = __uint_as_float(a1[0]) + __uint_as_float(a1[1]);
    const auto b0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(u), __float_as_uint(u), false, false);
    const auto b1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    u = __uint_as_float(b0[0]) + __uint_as_float(b0[1]);
    v = __uint_as_float(b1[0]) + __uint_as_float(b1[1]);
    u = u + dppf<0x128>(u);
    v = v + dppf<0x128>(v);
    u = u + dppf<0x124>(u);
    v = v + dppf<0x124>(v);
    u = u + dppf<0x4E>(u);
    v = v + dppf<0x4E>(v);
    u = u + dppf<0xB1>(u);
    v = v + dppf<0xB1>(v);
}
__device__ __forceinline__ float lane_f(float v, int l) {   // wave-uniform l
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

__device__ __forceinline__ float pat2(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float a = mx == 0.0f ? 0.0f : mn / mx;
    const float s = a * a;
    float r = fmaf(fmaf(fmaf(fmaf(fmaf(-0.0117212f, s, 0.05265332f), s, -0.11643287f), s, 0.19354346f), s,
                        -0.33262347f), s, 0.99997726f) * a;
    if (ay > ax) r = 1.57079637f - r;
    if (x < 0.0f) r = 3.14159274f - r;
    if (y < 0.0f) r = -r;
    return r;
}

// Cubic Lagrange interpolation of y (y[n] at w[n - w0]) at t and at t - 2 together: t - 2 is exact
// here (t < 2^22), so both share the fraction f and the four Lagrange weights -- computed once, the
// same bits either way.  (Measured and rejected: prefetching the next block's window at the position
// the current delta predicts, selected by the wave-uniform shift: 0.5 % slower -- the Gardner block is
// bound by its instruction chain, not by this LDS read.)
__device__ __forceinline__ void interp_pair(const float2 *w, int w0, float t, float2 &on, float2 &mid) {
    const float K6 = 1.0f / 6.0f;
    const float fi = floorf(t);
    const int i = (int)fi;
    const float f = t - fi;
    const float fm1 = f - 1.0f, fm2 = f - 2.0f, fp1 = f + 1.0f;
    const float cm = -(f * fm1 * fm2) * K6;
    const float c0 = (fp1 * fm1 * fm2) * 0.5f;
    const float c1 = -(fp1 * f * fm2) * 0.5f;
    const float c2 = (fp1 * f * fm1) * K6;
    auto one = [&](int j) -> float2 {
        const float2 a = w[j - 1 - w0], b = w[j - w0], c = w[j + 1 - w0], d = w[j + 2 - w0];
        float r = cm * a.x, q = cm * a.y;
        r = fmaf(c0, b.x, r); q = fmaf(c0, b.y, q);
        r = fmaf(c1, c.x, r); q = fmaf(c1, c.y, q);
        r = fmaf(c2, d.x, r); q = fmaf(c2, d.y, q);
        return make_float2(r, q);
    };
    on = one(i);
    mid = one(i - 2);
}

// interp_pair over a 512-sample LDS ring holding y[n] at ring[n & 511] (k_timing: the Gardner
// window staged from global memory a block ahead); the same operations as interp_pair
constexpr int TRING = 512;
__device__ __forceinline__ void interp_pair_ring(const float2 *w, float t, float2 &on, float2 &mid) {
    const float K6 = 1.0f / 6.0f;
    const float fi = floorf(t);
    const int i = (int)fi;
    const float f = t - fi;
    const float fm1 = f - 1.0f, fm2 = f - 2.0f, fp1 = f + 1.0f;
    const float cm = -(f * fm1 * fm2) * K6;
    const float c0 = (fp1 * fm1 * fm2) * 0.5f;
    const float c1 = -(fp1 * f * fm2) * 0.5f;
    const float c2 = (fp1 * f * fm1) * K6;
    auto one = [&](int j) -> float2 {
        const float2 a = w[(j - 1) & (TRING - 1)], b = w[j & (TRING - 1)], c = w[(j + 1) & (TRING - 1)],
                     d = w[(j + 2) & (TRING - 1)];
        float r = cm * a.x, q = cm * a.y;
        r = fmaf(c0, b.x, r); q = fmaf(c0, b.y, q);
        r = fmaf(c1, c.x, r); q = fmaf(c1, c.y, q);
        r = fmaf(c2, d.x, r); q = fmaf(c2, d.y, q);
        return make_float2(r, q);
    };
    on = one(i);
    mid = one(i - 2);
}

__device__ __forceinline__ float2 csqrt_p(float x, float y) {
    const float r = sqrtf(fmaf(x, x, y * y));
    if (r == 0.0f) return make_float2(0.f, 0.f);
    if (x >= 0.0f) {
        const float s = sqrtf((r + x) * 0.5f);
        return make_float2(s, y / (2.0f * s));
    }
    float s = sqrtf((r - x) * 0.5f);
    if (y < 0.0f) s = -s;
    return make_float2(y / (2.0f * s), s);
}

// CFO rotation conj((-Z/|Z|)^(1/4)) of Z = sum d^4 (oracle cfo_rotation).  Z goes with the 8th power
// of the input amplitude, so Zr^2 + Zi^2 overflows or underflows long before Z does: Z is first scaled
// by the exact power of two that brings max(|Zr|, |Zi|) into [0.5, 1) (v_frexp_exp / v_ldexp: no
// rounding).  Z = 0, infinite or NaN: no estimate, the identity rotation.  Once per channel.
__device__ __forceinline__ void cfo_rotation(float Zr, float Zi, float &rr, float &ri) {
    rr = 1.0f;
    ri = 0.0f;
    const float m = fmaxf(fabsf(Zr), fabsf(Zi));
    if (!(m > 0.0f && m <= FLT_MAX)) return;
    int e;
    (void)frexpf(m, &e);
    const float zr = ldexpf(Zr, -e), zi = ldexpf(Zi, -e);
    const float zm = sqrtf(fmaf(zr, zr, zi * zi));
    const float2 v = csqrt_p(-zr / zm, -zi / zm);
    const float2 w = csqrt_p(v.x, v.y);
    rr = w.x;
    ri = -w.y;
}

// The timing + decision stage for one channel.  timing_track runs on one wave (lane = 0..63): the
// Oerder-Meyr phase, block-Gardner tracking, and the CFO sums, which are folded into the Gardner
// blocks (lane l produces the symbols j = 64 b + l, ascending -- the order the oracle's CFO loop
// sums them in), so no second pass over d is needed; it leaves d_j in dp and returns the CFO
// rotation and soft scale.  timing_decide (the decision pass: rotation, int8 soft bits, hard
// dibits) is elementwise and is shared by `nw` waves.  y / dp may point to global memory (k_timing)
// or LDS (the fused demod); every cross-lane exchange in timing_track is a wave reduction or
// shuffle, so it needs no workgroup barrier.
struct TrackOut {
    int S;
    float rr, ri, sc, base, delta;
    int kstart, J0;   // first block's k; 1 when symbol 0 is the carried previous one (streaming)
    float pr, pi;     // the last symbol
};

// Streaming input of one channel's timing (tetra_etsi_track + the window's yoff): acq = 0 is the
// non-streaming receiver (Oerder-Meyr acquisition on the chunk, a new differential chain).
struct TrackIn {
    int acq;
    float base, delta, pr, pi;
    int yoff;
};
__device__ __forceinline__ TrackIn track_in(const tetra_etsi_track *t, int yoff) {
    if (!t) return TrackIn{0, 0.f, 0.f, 0.f, 0.f, 0};
    return TrackIn{t->acquired, t->base, t->delta, t->prev_re, t->prev_im, yoff};
}
// The state for the next chunk (oracle/etsi_oracle.c timing_core): the next symbol's base relative
// to this window's end, the loop offset and the last symbol.
__device__ __forceinline__ void track_store(tetra_etsi_track *t, const TrackIn &ti, const TrackOut &o, int M2) {
    if (M2 < 16) {
        if (ti.acq) t->base = ti.base + (float)(ti.yoff - M2);
        return;
    }
    if (ti.acq || o.S > 0) {
        t->base = o.base + (float)(4 * (o.kstart + o.S - o.J0) - M2);
        t->delta = o.delta;
        t->prev_re = o.pr;
        t->prev_im = o.pi;
        t->acquired = 1;
    }
}

// SPLIT: the CFO sums are left to a second wave (cfo_consumer) that follows the tracking through
// the LDS progress word *prog (symbols done | PROG_DONE at the end): off the serial tracking chain.
constexpr int PROG_DONE = 1 << 30;
// Oerder-Meyr part w for this lane: |y[n]|^2 summed over n = 64 b + lane, b in [w q4, (w + 1) q4),
// q4 = ceil(nb / 4) (loads issued 8 ahead; ascending order)
__device__ __forceinline__ float om_part(const float2 *y, int M2, int w, int lane) {
    const int nb = (M2 + 63) / 64, q4 = (nb + 3) / 4;
    const int n1 = min(64 * min((w + 1) * q4, nb), M2);
    float s = 0.f;
    for (int n0 = 64 * w * q4 + lane; n0 < n1; n0 += 8 * 64) {
        float2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = n0 + 64 * u < n1 ? y[n0 + 64 * u] : make_float2(0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (n0 + 64 * u < n1) s += fmaf(v[u].x, v[u].x, v[u].y * v[u].y);
    }
    return s;
}
// The four om_part sums of one lane with the quarters' loads interleaved (k_timing, y in global
// memory): OM_U loads of each quarter in flight together -- 4 OM_U -- instead of om_part's 8 of one
// quarter, so the pass waits on 4x fewer round trips; each quarter still sums in ascending n and the
// quarters are added in order, so the result is om_part(0) + .. + om_part(3) to the bit.
constexpr int OM_U = 4;
__device__ __forceinline__ float om_all(const float2 *y, int M2, int lane) {
    const int nb = (M2 + 63) / 64, q4 = (nb + 3) / 4;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < q4; i += OM_U) {
        float2 v[4][OM_U];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int n1 = min(64 * min((w + 1) * q4, nb), M2);
#pragma unroll
            for (int u = 0; u < OM_U; ++u) {
                const int n = 64 * (w * q4 + i + u) + lane;
                v[w][u] = (i + u < q4 && n < n1) ? y[n] : make_float2(0.f, 0.f);
            }
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int n1 = min(64 * min((w + 1) * q4, nb), M2);
#pragma unroll
            for (int u = 0; u < OM_U; ++u) {
                const int n = 64 * (w * q4 + i + u) + lane;
                if (i + u < q4 && n < n1) s[w] += fmaf(v[w][u].x, v[w][u].x, v[w][u].y * v[w][u].y);
            }
        }
    }
    return ((s[0] + s[1]) + s[2]) + s[3];
}

// RING (k_timing, y in global memory): the Gardner loop reads y from a 512-sample LDS ring (4 KB: eight
// one-wave workgroups per SIMD still fit) filled a block ahead -- block b needs y[4 kb - 5, 4 kb + 260)
// (|delta| <= 1.5, the cubic window), the ring holds [0, 320) before the loop, and block b first writes
// the 256 samples the previous block loaded into registers, [320 + 256 (b - 1), 320 + 256 b) (over
// [256 b - 448, 256 b - 192), which no later block reads), then loads the next 256: each block's window
// reads wait on LDS, not on L2 / HBM.  (A continued stream's first symbol can lie further into y: all of
// these indices are then counted from the ring's origin `org`, see below.)  Same interpolation
// arithmetic, same bits.  RING = 2 keeps two blocks' loads in flight in registers (pre, pre2: the
// ring's contents at every block are the same).
// LEAN (k_timing): the Oerder-Meyr pass by om_all (all quarters' loads together) instead of om_part per
// quarter, and no d_j stores -- the decision pass recomputes d_j from the stored symbols (timing_decide_sym).
// OMC (k_timing's OMG form): the Oerder-Meyr class sums are given (omc = A0..A3, wave-uniform) --
// the wideband resampler formed their group partials -- and the pass over y is skipped.
template <bool SPLIT = false, int RING = 0, bool LEAN = false, bool OMC = false>
__device__ __forceinline__ TrackOut timing_track(const float2 *y, int M2, float gain, float soft_scale, float2 *sp,
                                                 float2 *dp, int smax, int lane, int *prog = nullptr,
                                                 const float *om = nullptr, float2 *ring = nullptr,
                                                 uint32_t *clk = nullptr, float4 omc = float4{},
                                                 TrackIn ti = TrackIn{}) {
    TrackOut o{0, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, 0, 0.0f, 0.0f};
    if (M2 < 16) {
        if constexpr (SPLIT) {
            if (lane == 0) __hip_atomic_store(prog, PROG_DONE, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        return o;
    }
    // Oerder-Meyr: class sums of |y|^2 over n mod 4, per lane as four partial sums over quarters of
    // the blocks added in order (om_part; the oracle's order) -- precomputed by four waves (om)
    // or computed here one after the other.  Streaming with the loop acquired: no acquisition, the
    // carried base (plus the window's yoff) and delta continue (oracle timing_core)
    float A0 = 0.f, A1 = 0.f, A2 = 0.f, A3 = 0.f;
    if (ti.acq) {
    } else if constexpr (OMC) {
        A0 = omc.x;
        A1 = omc.y;
        A2 = omc.z;
        A3 = omc.w;
    } else {
        float s;
        if (om) {
            s = om[lane];
#pragma unroll
            for (int w = 1; w < 4; ++w) s = s + om[64 * w + lane];
        } else if constexpr (LEAN) {
            s = om_all(y, M2, lane);
        } else {
            s = om_part(y, M2, 0, lane);
#pragma unroll
            for (int w = 1; w < 4; ++w) s = s + om_part(y, M2, w, lane);
        }
        s = bfly<4>(s);
        A0 = lane_f(s, 0);
        A1 = lane_f(s, 1);
        A2 = lane_f(s, 2);
        A3 = lane_f(s, 3);
    }
    if (clk && lane == 0) clk[1] = (uint32_t)wall_clock64();   // probe: the Oerder-Meyr pass done
    float base, delta;
    int kstart;
    const int J0 = ti.acq ? 1 : 0;
    if (ti.acq) {
        base = ti.base + (float)ti.yoff;
        delta = ti.delta;
        kstart = 0;
    } else {
        const float Xr = A0 - A2, Xi = A3 - A1;
        const float p = -0.63661977236758134f * pat2(Xi, Xr);
        base = p < 0.0f ? p + 4.0f : p;
        if (base >= 4.0f) base -= 4.0f;
        kstart = base >= 3.0f ? 0 : 1;
        delta = 0.0f;
    }
    int S = J0;   // symbol 0 of a continued stream is the carried last symbol
    float2 prev = J0 ? make_float2(ti.pr, ti.pi) : make_float2(0.f, 0.f);
    bool have_prev = J0 != 0;
    if (J0 && lane == 0 && smax > 0) sp[0] = prev;
    float zr = 0.f, zi = 0.f, am = 0.f;   // CFO sums over this lane's d_j
    int rel = -1;   // SPLIT: progress not yet released (published after the next block's LDS reads)
    float2 pre[4], pre2[4];   // RING: the next block's 256 samples in flight (RING 2: and the one after)
    // RING: the ring's loads go through a buffer resource over y (past M2 they return 0) and the symbol
    // stores through one over sp (past smax they are dropped), both without branches: hipcc then
    // counts the wave's memory operations exactly and waits at a block's ring writes only for the
    // loads it needs, not (vmcnt(0)) for the previous block's symbol stores as well
    typedef unsigned u2v __attribute__((ext_vector_type(2)));
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2 *>(y), 0, 8 * M2, 0x00020000);
    const __amdgpu_buffer_rsrc_t sps = __builtin_amdgcn_make_buffer_rsrc(sp, 0, 8 * smax, 0x00020000);
    auto ld = [&](int n) -> float2 {
        if constexpr (RING > 0) {
            const u2v v = __builtin_amdgcn_raw_buffer_load_b64(yrs, 8 * n, 0, 0);
            return make_float2(__uint_as_float(v.x), __uint_as_float(v.y));
        } else {
            return n < M2 ? y[n] : make_float2(0.f, 0.f);
        }
    };
    // RING, streaming: the first symbol is at base = the carried base + yoff, and yoff goes up to
    // TETRA_ETSI_MARGIN + the outputs of one window period (2 up: 151 at 127 kSps), past what a ring
    // filled from y[0] holds for block 0.  The ring starts at org instead, a multiple of 4 with
    // base - org in [8, 12) (0 while base < 8, and without a carried loop, where base < 4): block b
    // then reads y[org + 256 b + 3, org + 256 b + 268), inside the [org + 256 b - 192, org + 256 b + 320)
    // the ring holds.
    int org = 0;
    if constexpr (RING > 0) {
        if (ti.acq) org = max(0, (int)base - 8) & ~3;
#pragma unroll
        for (int u = 0; u < 5; ++u) ring[(org + 64 * u + lane) & (TRING - 1)] = ld(org + 64 * u + lane);
#pragma unroll
        for (int u = 0; u < 4; ++u) pre[u] = ld(org + 320 + 64 * u + lane);
        if constexpr (RING > 1) {
#pragma unroll
            for (int u = 0; u < 4; ++u) pre2[u] = ld(org + 576 + 64 * u + lane);
        }
    }
    for (int kb = kstart;; kb += 64) {
        if constexpr (RING > 0) {
            if (kb != kstart) {   // the previous block's loads: y[320 + 256 (b - 1) ...)
                const int n0 = org + 320 + 4 * (kb - kstart) - 256;
#pragma unroll
                for (int u = 0; u < 4; ++u) ring[(n0 + 64 * u + lane) & (TRING - 1)] = pre[u];
                if constexpr (RING > 1) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        pre[u] = pre2[u];
                        pre2[u] = ld(n0 + 512 + 64 * u + lane);
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) pre[u] = ld(n0 + 256 + 64 * u + lane);
                }
            }
        }
        const float off = base + delta;
        const float t = (float)(4 * (kb + lane)) + off;
        const bool valid = (t - 3.0f >= 0.0f) && (t + 2.0f <= (float)(M2 - 1)) && (S + lane < smax);
        const unsigned long long bal = __ballot(!valid);
        const int nv = bal ? (__ffsll((long long)bal) - 1) : 64;
        const bool act = lane < nv;
        float2 on = make_float2(0.f, 0.f), mid = make_float2(0.f, 0.f);
        if constexpr (SPLIT) {
            // y in LDS: every lane interpolates, so the window reads do not wait for the ballot
            // (a lane past nv reads in or past the workgroup's LDS -- past it reads return 0 -- and
            // its values are dropped below)
            float2 a, b;
            interp_pair(y, 0, t, a, b);
            asm volatile("" ::"v"(a.x), "v"(a.y), "v"(b.x), "v"(b.y));   // computed here, not sunk into the branch
            if (act) {
                on = a;
                mid = b;
            }
            if (rel >= 0 && lane == 0)   // the previous block's d_j: its stores completed before these reads
                __hip_atomic_store(prog, rel, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else if constexpr (RING > 0) {
            if (act) interp_pair_ring(ring, t, on, mid);
        } else {
            if (act) interp_pair(y, 0, t, on, mid);
        }
        float2 pv = make_float2(dppf<0x138>(on.x), dppf<0x138>(on.y));   // wave_shr:1 (lane 0 replaced below)
        bool hp_ = true;
        if (lane == 0) { pv = prev; hp_ = have_prev; }
        float ev = 0.f, pw = 0.f;
        if (act) {
            pw = fmaf(on.x, on.x, on.y * on.y);
            if (hp_) {
                const float dr = on.x - pv.x, di = on.y - pv.y;
                ev = fmaf(dr, mid.x, di * mid.y);
                const int j = S + lane;
                const float xr = fmaf(on.x, pv.x, on.y * pv.y), xi = fmaf(on.y, pv.x, -(on.x * pv.y));
                if constexpr (!LEAN) dp[j - 1] = make_float2(xr, xi);
                if constexpr (!SPLIT) {
                    // CFO: 4th power and magnitude of d_j (j = lane mod 64, ascending: the oracle's order)
                    const float sr = fmaf(xr, xr, -(xi * xi)), si = (xr * xi) * 2.0f;
                    const float qr = fmaf(sr, sr, -(si * si)), qi = (sr * si) * 2.0f;
                    zr += qr;
                    zi += qi;
                    am += sqrtf(fmaf(xr, xr, xi * xi));
                }
            }
            if constexpr (RING == 0) sp[S + lane] = on;
        }
        // RING: every lane stores (a lane past nv stores 0 at S + lane >= the final S, or nothing past smax)
        if constexpr (RING > 0)
            __builtin_amdgcn_raw_buffer_store_b64(u2v{__float_as_uint(on.x), __float_as_uint(on.y)}, sps, 8 * (S + lane),
                                                  0, 0);
        if (nv > 0) {
            float E = ev, W = pw;
            wave_sum2(E, W);
            if (W > 0.0f) delta = delta - gain * (E / W);
            if (delta > 1.5f) delta = 1.5f;
            if (delta < -1.5f) delta = -1.5f;
            prev = make_float2(lane_f(on.x, nv - 1), lane_f(on.y, nv - 1));
            have_prev = true;
        }
        S += nv;
        if constexpr (SPLIT) rel = S;   // d_j, j < S, are in dp: released to the CFO wave next block
        if (nv < 64) break;
    }
    if constexpr (SPLIT) {   // the last block's d_j, and the end
        if (lane == 0) __hip_atomic_store(prog, S | PROG_DONE, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    o.S = S;
    o.base = base;
    o.delta = delta;
    o.kstart = kstart;
    o.J0 = J0;
    o.pr = prev.x;
    o.pi = prev.y;
    if constexpr (SPLIT) return o;   // rr, ri, sc: cfo_consumer's
    // CFO rotation conj((-Z/|Z|)^(1/4)) and the soft scale from the mean |d|
    const float Zr = wave_sum(zr), Zi = wave_sum(zi), A = wave_sum(am);
    float rr, ri;
    cfo_rotation(Zr, Zi, rr, ri);
    o.rr = rr;
    o.ri = ri;
    o.sc = (S > 1 && A > 0.0f) ? soft_scale / (A / (float)(S - 1)) : 0.0f;
    return o;
}

// The CFO half of timing_track<false>, on a second wave while timing_track<true> tracks: lane l
// sums the 4th powers and magnitudes of d_j, j = l mod 64, block after block as the progress word
// releases them -- the same per-lane order, so the same bits -- then the rotation and the soft
// scale into *o (rr, ri, sc).
__device__ __forceinline__ void cfo_consumer(const float2 *dp, float soft_scale, int *prog, TrackOut *o, int lane,
                                             int j0 = 0) {
    // lane l sums d_j for j = j0 + l mod 64 (j0 = 1 when symbol 0 is a continued stream's carried one):
    // the tracking wave's lane order
    float zr = 0.f, zi = 0.f, am = 0.f;
    int jb = j0, S = 0;
    for (;;) {
        const int v = __hip_atomic_load(prog, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
        S = v & (PROG_DONE - 1);
        for (; jb < S; jb += 64) {
            const int j = jb + lane;
            if (j >= 1 && j < S) {
                const float2 d = dp[j - 1];
                const float xr = d.x, xi = d.y;
                const float sr = fmaf(xr, xr, -(xi * xi)), si = (xr * xi) * 2.0f;
                const float qr = fmaf(sr, sr, -(si * si)), qi = (sr * si) * 2.0f;
                zr += qr;
                zi += qi;
                am += sqrtf(fmaf(xr, xr, xi * xi));
            }
        }
        if (v & PROG_DONE) break;
        __builtin_amdgcn_s_sleep(1);
    }
    const float Zr = wave_sum(zr), Zi = wave_sum(zi), A = wave_sum(am);
    float rr, ri;
    cfo_rotation(Zr, Zi, rr, ri);
    if (lane == 0) {
        o->rr = rr;
        o->ri = ri;
        o->sc = (S > 1 && A > 0.0f) ? soft_scale / (A / (float)(S - 1)) : 0.0f;
    }
}

// Decision pass over d_j, j in [1, S): wave w of nw takes the 64-symbol blocks w, w + nw, ...
__device__ __forceinline__ void timing_decide(const TrackOut &o, const float2 *dp, int8_t *sb, uint8_t *hp, int w,
                                              int nw, int lane) {
    for (int j0 = 1 + 64 * w + lane; j0 < o.S; j0 += 4 * 64 * nw) {
        float2 dv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) dv[u] = j0 + 64 * nw * u < o.S ? dp[j0 + 64 * nw * u - 1] : make_float2(0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + 64 * nw * u;
            if (j >= o.S) break;
            const float2 d = dv[u];
            const float xr = fmaf(d.x, o.rr, -(d.y * o.ri)), xi = fmaf(d.x, o.ri, d.y * o.rr);
            float q1 = rintf(xi * o.sc), q2 = rintf(xr * o.sc);
            q1 = q1 > 127.f ? 127.f : (q1 < -127.f ? -127.f : q1);
            q2 = q2 > 127.f ? 127.f : (q2 < -127.f ? -127.f : q2);
            sb[2 * (j - 1)] = (int8_t)q1;
            sb[2 * (j - 1) + 1] = (int8_t)q2;
            hp[j - 1] = (uint8_t)(((xi < 0.0f) << 1) | (xr < 0.0f));
        }
    }
}

// timing_decide with d_j = s_j conj(s_{j-1}) recomputed from the stored symbols sp -- the same fmas on
// the same values the tracking loop formed it from, so the same bits (k_timing LEAN: d_j is not stored)
__device__ __forceinline__ void timing_decide_sym(const TrackOut &o, const float2 *sp, int8_t *sb, uint8_t *hp,
                                                  int lane) {
    for (int j0 = 1 + lane; j0 < o.S; j0 += 4 * 64) {
        float2 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + 64 * u;
            a[u] = j < o.S ? sp[j] : make_float2(0.f, 0.f);
            b[u] = j < o.S ? sp[j - 1] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + 64 * u;
            if (j >= o.S) break;
            const float2 on = a[u], pv = b[u];
            const float dx = fmaf(on.x, pv.x, on.y * pv.y), dy = fmaf(on.y, pv.x, -(on.x * pv.y));
            const float xr = fmaf(dx, o.rr, -(dy * o.ri)), xi = fmaf(dx, o.ri, dy * o.rr);
            float q1 = rintf(xi * o.sc), q2 = rintf(xr * o.sc);
            q1 = q1 > 127.f ? 127.f : (q1 < -127.f ? -127.f : q1);
            q2 = q2 > 127.f ? 127.f : (q2 < -127.f ? -127.f : q2);
            sb[2 * (j - 1)] = (int8_t)q1;
            sb[2 * (j - 1) + 1] = (int8_t)q2;
            hp[j - 1] = (uint8_t)(((xi < 0.0f) << 1) | (xr < 0.0f));
        }
    }
}

}  // namespace

// --------------------------------------------------------------------------- host side (etsi_timing.hip)
int timing_probe();
void launch_track_skip(tetra_ctx *ctx, tetra_etsi_track *tr, size_t C, int yoff, int M2);

// The timing stage's outputs as every entry point stages them, in this order (the order of the
// Staging calls decides the slots): C rows of `stride` symbols, soft bits (2 per symbol) and hard
// dibits, nsym per row, and the optional diagnostics.
struct DemodOut {
    float2 *sym;
    int8_t *softbits;
    uint8_t *hard;
    int32_t *nsym;
    float4 *diag;
    bool ok() const { return sym && softbits && hard && nsym; }
};
DemodOut stage_demod_out(Staging &st, void *soft, int8_t *softbits, uint8_t *hard, int32_t *nsym, float *diag,
                         size_t C, size_t stride);

// The parts of a k_timing launch only some callers have.
struct TimingOpt {
    tetra_etsi_track *track = nullptr;   // streaming: the channels' timing state,
    int yoff = 0, ostride = 0;           // the first new output of the window, the output rows' stride (0: smax)
    const float4 *om = nullptr;          // the _om forms: the resampler's group partials,
    int ngrp = 0, U = 0;                 // ngrp float4 per carrier row, U samples per group
    int nchunk = 0, cstride = 0;         // chunked rows: chunks per carrier row, their stride (0: rows of M2)
    long rowlen = 0;                     // and the carrier rows' length
};
void launch_timing(tetra_ctx *ctx, const tetra_etsi_plan *P, const float2 *y, size_t C, size_t M2, const DemodOut &o,
                   float2 *dscr, size_t smax, const TimingOpt &t = TimingOpt{});
