// etsi_chanfilt.hip -- the ETSI channel filter with workgroup-wide tiles.
//
//   k_chanfilt   stage 1: 48-tap decimate-by-10 FIR (2.4 MSps -> 240 kHz), stage 2: polyphase RRC
//                (alpha 0.35, 321 taps at 720 kHz) resampler x3/10 -> 72 kHz = 4 samples/symbol, in
//                workgroup-wide 2560-sample tiles (barrier per tile, stage 2 every 8 tiles): SC16 rows
//                that are not a multiple of four samples (y round-tripped through L2, four workgroups
//                per CU; fused with the timing stage where y and its scratch fit the freed LDS) and
//                chunks longer than YLDS outputs.  Every other chunk takes k_chanfilt_r
//                (etsi_chanfilt_r.hip), which produces the same fma chains.
#include "etsi_chanfilt.h"

namespace {

// The input tile is a linear float4 image (2 samples per entry, ds_write_b128 / ds_read_b128: a
// 20-dword lane stride is conflict-free for b128's lane groups).  Stage-1 outputs x240[k] go to a
// linear buffer lin[k - kbase]; after each stage-2 burst the still-needed tail is moved to its
// front (kbase = 10 u_done), so stage 2's operand reads are base + immediate offset.
constexpr int PFD = 2;          // k_chanfilt: input tiles in flight per workgroup (register prefetch
                                // depth, pa/pb; 3 and 4 measured no faster)

// SC16 is held to 128 VGPRs: four workgroups per CU (its LDS allows four; at 158-161 VGPRs it ran at
// three, 1.10 -> 1.57 ms per batch)
template <typename In> constexpr int cf_waves() { return std::is_same<In, float4>::value ? 2 : 4; }
template <typename In, bool FUSE>
__global__ __launch_bounds__(256, cf_waves<In>()) void k_chanfilt(const In *__restrict__ iq, long N, int M1, int M2,
                                                  const float *__restrict__ h1, const float *__restrict__ afrag,
                                                  float2 *__restrict__ y, TimingOut to, long ld) {
    constexpr bool YL = std::is_same<In, float4>::value;
    // cf32 keeps y in LDS (yb, 72 KB: two workgroups per CU, no y traffic); SC16 streams half the
    // bytes per sample and is bound by the workgroup's own LDS/issue chain instead, so it keeps
    // only the image and the stage-1 buffer (39 KB: four workgroups per CU) and sends y through
    // HBM/L2
    constexpr int LR = CF_LR;
    __shared__ float4 lds[(YL ? CF_LDS4 + YLDS / 2 : CF_LDS4) + 12];
    float4 *xin = lds;
    float2 *lin = reinterpret_cast<float2 *>(lds + XIN4);
    float *yb = reinterpret_cast<float *>(lds + CF_LDS4);   // YL only: y as (re, im) floats
    // the 48 stage-1 taps in LDS, read as broadcast float4s beside the samples: as scalar operands
    // hipcc re-loads them every tile (SGPR pressure), and those scalar loads share lgkmcnt with the
    // LDS reads, so each sample read was waited for right before its use (one or two in flight)
    float4 *htap = lds + (YL ? CF_LDS4 + YLDS / 2 : CF_LDS4);
    if (threadIdx.x < 12)
        htap[threadIdx.x] = make_float4(h1[4 * threadIdx.x], h1[4 * threadIdx.x + 1], h1[4 * threadIdx.x + 2],
                                        h1[4 * threadIdx.x + 3]);
    const int ch = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const In *xp = iq + (size_t)ch * (ld / 2);   // N, ld even: 2 complex samples per load; rows ld apart
    float2 *yp = y + (size_t)ch * M2;           // (YL && FUSE: unused)
    int ybase = 0;   // y index of yb[0]
    // Stage-2 outputs collect in yb and go out in one coalesced burst when the channel is done (or
    // when YLDS fills): stores interleaved with the input stream cost ~0.3 ms per 8192-channel
    // batch at two workgroups per CU (HBM read/write turnarounds, and store acks inside the
    // prefetch's in-order vmcnt).
    auto flush = [&](int mend) {
        for (int i = tid; i < mend - ybase; i += 256) yp[ybase + i] = make_float2(yb[2 * i], yb[2 * i + 1]);
        ybase = mend;
    };
    float at[S2K];   // this lane's A fragments
#pragma unroll
    for (int k = 0; k < S2K; ++k) at[k] = afrag[64 * k + lane];
    // stage 2 reads whole windows, zero taps included: every entry must be finite
    for (int i = tid; i < LR; i += 256) lin[i] = make_float2(0.f, 0.f);
    int kbase = 0;   // x240 index of lin[0]
    // register prefetch PFD tiles deep (40 KiB in flight per workgroup): tile t's samples
    // [2560 t, 2560 t + 2560) land at image sample HALO + i
    // Loads are unconditional (index clamped) so the wait before a tile's LDS write can leave the
    // next tile's loads in flight.  Clamped samples past the end only feed stage-1 outputs k >= M1,
    // which are never computed (10 (M1-1) + 47 <= N-1).
    const long nq = N / 2;
    auto load_tile = [&](In (&pf)[5], int t) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const long q = (long)t * (TILE_IN / 2) + r * 256 + tid;   // sample-pair index
            pf[r] = ld_nt(xp + min(q, nq - 1));   // streamed once: nt (common.h)
        }
    };
    int u_done = 0;   // stage-2 output triples [0, u_done) are stored
    auto tile = [&](int t, In (&pf)[5]) __attribute__((always_inline)) {
        const int kfirst = TILE_K * t - 4;   // stage-1 output of thread 0 in this tile
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const float4 v = pair_f32(pf[r]);
            xin[HALO / 2 + r * 256 + tid] = make_float4(v.x, v.y, v.z, v.w);
        }
        // keep the re-load after the LDS writes so pf's registers are reused in place (otherwise
        // the scheduler hoists it and the loop latch copies registers under a full vmcnt(0))
        __builtin_amdgcn_sched_barrier(0);
        load_tile(pf, t + PFD);   // tile t+PFD in flight during compute (t+1.. already are)
        __syncthreads();
        // stage 1: x240[k] = sum_j h1[j] * x[10k + j], k = kfirst + tid; x[10k + j] is sample
        // 10 tid + 8 + j of the image
        const int k = kfirst + tid;
        if (k >= 0 && k < M1) {
            const float4 *w = xin + 5 * tid + 4;
            pf2 a = {0.f, 0.f};
            if constexpr (YL) {   // three groups of 16 taps, the next group's reads in flight
                float4 ta[4], xa[8], tb[4], xb[8];
                auto rd = [&](float4 (&T)[4], float4 (&X)[8], int g) __attribute__((always_inline)) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        T[i] = htap[4 * g + i];
                        X[2 * i] = w[8 * g + 2 * i];
                        X[2 * i + 1] = w[8 * g + 2 * i + 1];
                    }
                };
                auto fm = [&](const float4 (&T)[4], const float4 (&X)[8]) __attribute__((always_inline)) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float4 t4 = T[i], x0 = X[2 * i], x1 = X[2 * i + 1];
                        a = pfma(t4.x, pf2{x0.x, x0.y}, a);
                        a = pfma(t4.y, pf2{x0.z, x0.w}, a);
                        a = pfma(t4.z, pf2{x1.x, x1.y}, a);
                        a = pfma(t4.w, pf2{x1.z, x1.w}, a);
                    }
                };
                rd(ta, xa, 0);
                rd(tb, xb, 1);
                __builtin_amdgcn_sched_barrier(0);
                fm(ta, xa);
                __builtin_amdgcn_sched_barrier(0);
                rd(ta, xa, 2);
                __builtin_amdgcn_sched_barrier(0);
                fm(tb, xb);
                __builtin_amdgcn_sched_barrier(0);
                fm(ta, xa);
            } else {   // SC16 keeps the scalar taps (VGPR budget, below; LDS taps read two quads ahead
                       // of the chain measured 3 % slower: 1.20 -> 1.24 ms per pipelined SC16 step)
#pragma unroll
                for (int jj = 0; jj < 24; ++jj) {
                    const float4 v = w[jj];
                    a = pfma(h1[2 * jj], pf2{v.x, v.y}, a);
                    a = pfma(h1[2 * jj + 1], pf2{v.z, v.w}, a);
                }
            }
            lin[k - kbase] = make_float2(a.x, a.y);
        }
        __syncthreads();
        // halo for the next tile: image samples [0, 48) = this tile's [2560, 2608)
        if (tid < HALO / 2) xin[tid] = xin[TILE_IN / 2 + tid];
        const int kav = min(kfirst + TILE_K - 1, M1 - 1);   // last stage-1 output available
        const bool last = kav == M1 - 1;
        if (t % S2_EVERY == S2_EVERY - 1 || last) {
            // stage 2: triples u whose three outputs have all taps available (all of them at the end)
            const int num = 3 * kav + 2 - 320;   // largest m with floor((320 + 10m)/3) <= kav
            const int m_hi = num >= 0 ? min(num / 10, M2 - 1) : -1;
            const int u_hi = last ? (M2 - 1) / 3 : (m_hi >= 2 ? (m_hi - 2) / 3 : -1);
            const int nt = u_hi >= u_done ? (u_hi - u_done + S2T) / S2T : 0;   // MFMA tiles
            const int mend = min(3 * (u_hi + 1), M2);
            if (YL && nt > 0 && mend - ybase > YLDS) {   // this burst would not fit
                flush(3 * u_done);
                __syncthreads();
            }
            // columns: lane & 15 = 2 seg + comp; k-group lane >> 4.  Tile pairs (2p, 2p + 1) go to
            // wave p % 4: two independent accumulators per wave cover the MFMA's latency.
            const int kg = lane >> 4, seg = (lane & 15) >> 1, comp = lane & 1;
            const float *lf = reinterpret_cast<const float *>(lin);
            float *ys = YL ? yb : reinterpret_cast<float *>(xin + HALO / 2);   // !YL: staged, stored below
            const int yo = YL ? ybase : 3 * u_done;
            for (int p = wv; 2 * p < nt; p += 4) {
                const int U0 = u_done + 2 * p * S2T + S2Q * seg, U1 = U0 + S2T;
                // a column past u_hi reads the buffer's start instead (finite, never stored)
                const int b0 = U0 <= u_hi ? 2 * (10 * U0 - kbase + kg) + comp : 2 * kg + comp;
                const int b1 = U1 <= u_hi ? 2 * (10 * U1 - kbase + kg) + comp : 2 * kg + comp;
                f4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
                if constexpr (YL) {
                    // B operands a third of the chain ahead (hipcc otherwise waits lgkmcnt(0), one
                    // LDS round trip, before each MFMA pair).  Not for SC16: the 26 extra VGPRs
                    // take it from 120 to 161, four workgroups per CU to three (1.10 -> 1.57 ms)
                    float bv0[S2K], bv1[S2K];
#pragma unroll
                    for (int s3 = 0; s3 < 3; ++s3) {
#pragma unroll
                        for (int s2 = 13 * s3; s2 < 13 * s3 + 13; ++s2) {
                            bv0[s2] = lf[b0 + 8 * s2];
                            bv1[s2] = lf[b1 + 8 * s2];
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int s2 = 13 * s3; s2 < 13 * s3 + 13; ++s2) {
                            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(at[s2], bv0[s2], c0, 0, 0, 0);
                            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(at[s2], bv1[s2], c1, 0, 0, 0);
                        }
                    }
                } else {
#pragma unroll
                    for (int s2 = 0; s2 < S2K; ++s2) {
                        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(at[s2], lf[b0 + 8 * s2], c0, 0, 0, 0);
                        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(at[s2], lf[b1 + 8 * s2], c1, 0, 0, 0);
                    }
                }
                // D: this lane holds rows i = 4 kg + r of its column; output m = 3 U + i
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 4 * kg + r, q = i / 3;
                    if (i < 15) {
                        const int m0 = 3 * U0 + i, m1 = 3 * U1 + i;
                        if (U0 + q <= u_hi && m0 < M2) ys[2 * (m0 - yo) + comp] = c0[r];
                        if (U1 + q <= u_hi && m1 < M2) ys[2 * (m1 - yo) + comp] = c1[r];
                    }
                }
            }
            if constexpr (!YL) {
                if (nt > 0) {   // coalesced store of this burst's outputs y[3 u_done, mend)
                    __syncthreads();
                    // sc1 (copy_out): 1.11 -> 1.09 ms per SC16 batch, same box
                    copy_out(reinterpret_cast<uint8_t *>(yp + yo), reinterpret_cast<const uint8_t *>(ys), 8 * (mend - yo), tid);
                }
            }
            if (u_hi + 1 > u_done) u_done = u_hi + 1;
            if (!last) {
                // keep x240[10 u_done, kav] (the next triples' windows) at the buffer's front
                const int from = 10 * u_done - kbase, cnt = kav + 1 - 10 * u_done;
                __syncthreads();
                const float2 v = tid < cnt ? lin[from + tid] : make_float2(0.f, 0.f);
                __syncthreads();
                if (tid < cnt) lin[tid] = v;
                kbase = 10 * u_done;
            }
        }
        __syncthreads();
    };
    const int ntile = (M1 + 4 + TILE_K - 1) / TILE_K;   // tiles with kfirst < M1
    // two register sets, explicitly (a pr[PFD][5] array with unrolled loops over it cost 22-30 VGPRs:
    // SC16 at 142 instead of 120 lost its fourth workgroup per CU)
    static_assert(PFD == 2, "pa / pb below");
    In pa[5], pb[5];
    load_tile(pa, 0);
    load_tile(pb, 1);
    int t = 0;
    for (; t + 1 < ntile; t += 2) {
        tile(t, pa);
        tile(t + 1, pb);
    }
    if (t < ntile) tile(t, pa);
    // the last tile ended with a barrier
    if constexpr (FUSE) {
        const float2 *ly = reinterpret_cast<const float2 *>(yb);   // YL: yb holds y[0, M2)
        float2 *scr = reinterpret_cast<float2 *>(xin);
        if constexpr (!YL) {
            // y (this workgroup's stores) back into LDS, the timing scratch after it (the launch
            // guarantees M2 + smax <= CF_LDS2_SC16).  Workgroup-scope fence: the stores and the loads
            // share this CU's L1 (a device-scope fence would write back the whole L2 per channel).
            __threadfence_block();
            __syncthreads();
            float2 *yl = reinterpret_cast<float2 *>(lds);
            for (int i0 = tid; i0 < M2; i0 += 4 * 256) {
                float2 v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = i0 + 256 * e < M2 ? yp[i0 + 256 * e] : make_float2(0.f, 0.f);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (i0 + 256 * e < M2) yl[i0 + 256 * e] = v[e];
            }
            __syncthreads();
            ly = yl;
            scr = yl + M2;
        }
        __shared__ TrackOut tro;
        __shared__ int prog;
        timing_tail(ly, scr, to, M2, ch, tid, &tro, &prog);
    } else if constexpr (YL) {
        flush(M2);
    }
}

}  // namespace

// cf32 has no fused form here: a cf32 chunk whose y fits the fused tail's LDS (M2 <= YLDS) is always
// k_chanfilt_r's (etsi_demod.hip fused_fits).
const void *chanfilt_fn(int fmt, bool fused) {
    if (fmt == TETRA_SC16)
        return fused ? reinterpret_cast<const void *>(&k_chanfilt<uint2, true>)
                     : reinterpret_cast<const void *>(&k_chanfilt<uint2, false>);
    return fused ? nullptr : reinterpret_cast<const void *>(&k_chanfilt<float4, false>);
}
