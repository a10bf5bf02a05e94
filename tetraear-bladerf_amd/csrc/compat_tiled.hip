// compat_tiled.hip -- decimate's fp32 sosfiltfilt cut into time tiles, bit-identical to the
// sequential kernels of compat_decimate.hip (TETRA_COMPAT_TILED, opt-in).
//
// The cheby1(8) recursion forgets its start: run from an all-zero state TL_WARM samples early, its
// fp32 state is usually the sequential run's, bit for bit, by the time the tile begins.  That is
// checked, not trusted.  Per pass over ext[0, L) (forward) or the reversed forward output (backward),
// tiles [kT, min((k+1)T, L)), k = 0..K-1:
//   1. k_tl_spec: every tile of every stream at once.  Tile k starts at a = max(0, kT - W), from the
//      pass's exact start state zi * seq[0] when a == 0 and from zero otherwise, stores outputs only
//      for samples inside the tile, and records S_k (the 8 state words just before sample kT) and
//      E_k (just after the tile's last sample).
//   2. k_tl_resolve: per stream, in tile order.  E*_0 = E_0; if S_k equals E*_{k-1} as 32-bit
//      patterns (-0 != +0, NaN never equal: the safe side) then E*_k = E_k, else tile k is rerun from
//      E*_{k-1}, its outputs overwritten, and E*_k is the rerun's end state.
// By induction every stored output is the sequential run's.  W only sets how often step 2 reruns:
// never on noisy captures at the defaults (tools/compat_tile_sweep.py), always on noiseless input
// (constant rows, exact zeros after a burst), where the mode is as slow as the sequential one.
//
// Lanes are k_sos_fwd_bank's: section = DPP bank, the 4 lanes of a stream load 4 different 16-byte
// chunks, one 64-byte store per stream per 16 ticks; a tile is just another stream.  A tile's work
// is two phases of the same code -- warm-up [a, kT) storing nothing, then the tile -- each a few
// slow ticks up to an aligned start, then the unrolled batches.  The state snapshots are taken in
// the slow ticks around kT and the tile end, so the batches carry no extra work per tick.
#include "common.h"
#include "compat_sos.h"

namespace {

constexpr int TL_TILE = 8192;    // built-in tile length ...
constexpr int TL_WARM = 16384;   // ... and warm-up: 0 reruns in 8960 checked tiles of sweep_chunks, q = 7..10
constexpr int TL_PAD = 27;       // sosfiltfilt's padlen for 4 sections
constexpr int TL_MAXC = 64;      // past this the sequential kernels already fill the chip
constexpr int TL_B = 32;         // forward: ticks per batch
constexpr size_t TL_MAXK = 65536;   // tiles per stream (bounds the state arrays: 64 B per stream-tile and array)

struct TlGeo {
    int C, K, T, W;
    long N, L, Lp;
};

__host__ __device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ long lmax(long a, long b) { return a > b ? a : b; }

// scipy _arraytools.odd_ext of component `comp` of the complex row xr
__device__ __forceinline__ float tl_ext(const float *xr, int comp, long N, long j) {
    auto xat = [&](long n) { return xr[2 * n + comp]; };
    const float two = 2;
    if (j < TL_PAD) return two * xat(0) - xat(TL_PAD - j);
    if (j < TL_PAD + N) return xat(j - TL_PAD);
    return two * xat(N - 1) - xat(N - 2 - (j - TL_PAD - N));
}

// Forward: samples [a, hi) of one stream from the state in bq; outputs of [lo, hi) to the scratch
// row sp.  S: this lane's section state just before sample lo (a < lo), E: just after hi - 1.
// Every operation on a sample is k_sos_fwd_bank's.
__device__ __forceinline__ void tl_fwd_tile(const float *xr, int comp, long N, float *sp, int sec, bool own,
                                            Biquad<float> &bq, long a, long lo, long hi, float2 &S, float2 &E) {
    const bool st = own && sec == 3;
    float y = 0;
    auto tick = [&](long tau) __attribute__((always_inline)) {
        const float xin = tau < hi ? tl_ext(xr, comp, N, tau) : 0.f;
        const float left = from_left_bank(y);
        const long j = tau - sec;
        if (j >= a && j < hi) {
            y = bq.step(sec == 0 ? xin : left);
            if (st && j >= lo) sp[j] = y;
            if (j == lo - 1) S = make_float2(bq.z0, bq.z1);
            if (j == hi - 1) E = make_float2(bq.z0, bq.z1);
        }
    };
    constexpr int NW = TL_B / 8;   // 8-sample windows per batch
    const float *xw = xr + 4 * sec + comp;
    auto ld = [&](f4u (&v)[NW], long t0) __attribute__((always_inline)) {
        const float *src = xw + 2 * (t0 - TL_PAD);
#pragma unroll
        for (int k = 0; k < NW; ++k) v[k] = *reinterpret_cast<const f4u *>(src + 16 * k);
    };
    auto run = [&](f4u (&v)[NW], long t0, bool store) __attribute__((always_inline)) {
        float o[16];
#pragma unroll
        for (int u = 0; u < TL_B; ++u) {
            const f4u &pv = v[u >> 3];
            const float e = (u & 1) ? pv.z : pv.x;
            const float left = from_left_bank(y);
            float xin;
            switch ((u >> 1) & 3) {
                case 0: xin = bank0_from<0>(left, e); break;
                case 1: xin = bank0_from<1>(left, e); break;
                case 2: xin = bank0_from<2>(left, e); break;
                default: xin = bank0_from<3>(left, e); break;
            }
            y = bq.step(xin);   // every section active: t0 - 3 >= a
            o[u & 15] = y;
            if ((u & 15) == 15) {
                float w[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    w[i] = o[12 + i];
                    w[i] = dppf<0x10C, 0x1, false>(w[i], o[i]);       // bank 0 <- bank 3 (row_shl:12)
                    w[i] = dppf<0x108, 0x2, false>(w[i], o[4 + i]);   // bank 1 <- bank 3 (row_shl:8)
                    w[i] = dppf<0x104, 0x4, false>(w[i], o[8 + i]);   // bank 2 <- bank 3 (row_shl:4)
                }
                if (store) *reinterpret_cast<float4 *>(sp + (t0 + u - 18 + 4 * sec)) = float4{w[0], w[1], w[2], w[3]};
            }
        }
        // keep the unread elements live to here (see k_sos_fwd_bank)
#pragma unroll
        for (int k = 0; k < NW; ++k) asm volatile("" ::"v"(v[k]));
    };
    // A batch at t0 covers samples [t0 - 3, t0 + TL_B) over the four sections and loads row samples
    // [t0 - pad, t0 - pad + TL_B] (the imaginary lanes read one float past their window).  So it
    // starts once every section is inside [a, ..) and past the left extension, stops one sample
    // short of the row end, and leaves the samples lo - 1 and hi - 1 (the snapshots) to the slow
    // ticks.  The tile phase starts at lo + 3: its first store is sample lo, 16-byte aligned.
    const long interior = TL_PAD + N - 1;
    const long s0 = lmax(a + 3, TL_PAD), s1 = lmax(lo + 3, TL_PAD);
    const long l0 = lmin(lo - 1, interior), l1 = lmin(hi - 1, interior);
    long tau = a;
#pragma unroll 1
    for (int ph = 0; ph < 2; ++ph) {
        const long start = ph ? s1 : s0, limit = ph ? l1 : l0;
        const bool store = own && ph == 1;
        for (; tau < start; ++tau) tick(tau);
        if (limit - tau >= SOS_PD * TL_B) {
            f4u xs[SOS_PD][NW];
#pragma unroll
            for (int u = 0; u < SOS_PD; ++u) ld(xs[u], tau + u * TL_B);
            for (; tau + 2 * SOS_PD * TL_B <= limit; tau += SOS_PD * TL_B) {
#pragma unroll
                for (int u = 0; u < SOS_PD; ++u) {
                    run(xs[u], tau + u * TL_B, store);
                    __builtin_amdgcn_sched_barrier(0);
                    ld(xs[u], tau + (u + SOS_PD) * TL_B);
                }
            }
#pragma unroll
            for (int u = 0; u < SOS_PD; ++u) run(xs[u], tau + u * TL_B, store);
            tau += SOS_PD * TL_B;
        }
    }
    for (; tau < hi + 3; ++tau) tick(tau);
}

// Backward: samples [a, hi) of the reversed scratch row (sample kk is sp[L - 1 - kk]) from the state
// in bq; of [lo, hi) the outputs with t = L - 1 - kk - pad in [0, N) and t % QT == 0 go to op.
// Every operation on a sample is k_sos_bwd_bank's.
template <int QT>
__device__ __forceinline__ void tl_bwd_tile(const float *sp, long N, long L, float *op, size_t so, int sec, bool own,
                                            Biquad<float> &bq, long a, long lo, long hi, float2 &S, float2 &E) {
    const bool st = own && sec == 3;
    float y = 0;
    auto tick = [&](long tau) __attribute__((always_inline)) {
        const float xin = tau < hi ? sp[L - 1 - tau] : 0.f;
        const float left = from_left_bank(y);
        const long kk = tau - sec;
        if (kk >= a && kk < hi) {
            y = bq.step(sec == 0 ? xin : left);
            const long t = L - 1 - kk - TL_PAD;
            if (st && kk >= lo && t >= 0 && t < N && t % QT == 0) op[(size_t)(t / QT) * so] = y;
            if (kk == lo - 1) S = make_float2(bq.z0, bq.z1);
            if (kk == hi - 1) E = make_float2(bq.z0, bq.z1);
        }
    };
    constexpr int SB = QT * 16 / (QT % 16 == 0 ? 16 : QT % 8 == 0 ? 8 : QT % 4 == 0 ? 4 : QT % 2 == 0 ? 2 : 1);
    static_assert(SB % 16 == 0 && SB % QT == 0, "batch = lcm(16, QT)");
    constexpr int NL = SB / 16;
    // output index of section 3 at tick tt; with the batch start t0 chosen so that tcur(t0) % QT == PH,
    // tick u of a batch is an output tick iff u % QT == PH.  L - t0 is a multiple of 4 (aligned
    // loads), so tcur(t0) = L - t0 - 25 is odd: PH is a residue that 4 m - 25 can take mod QT.
    auto tcur = [&](long tt) { return L - 1 - (tt - 3) - TL_PAD; };
    constexpr int PH = QT % 2 ? 0 : QT % 8 == 0 ? 3 : 5 % QT;
    long s0 = a + 3;
    while ((L - s0) % 4) ++s0;
    const long b1 = lmax(lo, TL_PAD) + 3;   // past the right extension's outputs (t < N)
    long s1 = b1;
    while (((L - s1) % 4 || tcur(s1) % QT != PH) && s1 < b1 + 4 * QT) ++s1;
    const bool phased = (L - s1) % 4 == 0 && tcur(s1) % QT == PH;
    // batches leave samples lo - 1 and hi - 1 to the slow ticks, and stop while section 3's t >= 0
    const long l0 = lo - 1, l1 = phased ? lmin(hi - 1, L + 3 - TL_PAD) : 0;
    const float *sw = sp + L - 4 - 4 * sec;
    auto ld = [&](float4 (&v)[NL], long t0) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < NL; ++k) v[k] = *reinterpret_cast<const float4 *>(sw - t0 - 16 * k);
    };
    auto run = [&](float4 (&v)[NL], long t0, bool store) __attribute__((always_inline)) {
        const long tq0 = tcur(t0 + PH) / QT;   // wave-uniform per stream: output index of tick PH
#pragma clang loop unroll(full)
        for (int u = 0; u < SB; ++u) {
            const float4 &pv = v[u >> 4];
            const int el = 3 - (u & 3);
            const float e = el == 3 ? pv.w : el == 2 ? pv.z : el == 1 ? pv.y : pv.x;
            const float left = from_left_bank(y);
            float xin;
            switch ((u >> 2) & 3) {
                case 0: xin = bank0_from<0>(left, e); break;
                case 1: xin = bank0_from<1>(left, e); break;
                case 2: xin = bank0_from<2>(left, e); break;
                default: xin = bank0_from<3>(left, e); break;
            }
            y = bq.step(xin);
            if (u % QT == PH && store) op[(size_t)(tq0 - u / QT) * so] = y;
        }
    };
    long tau = a;
#pragma unroll 1
    for (int ph = 0; ph < 2; ++ph) {
        const long start = ph ? s1 : s0, limit = ph ? l1 : l0;
        const bool store = st && ph == 1;
        for (; tau < start; ++tau) tick(tau);
        if (limit - tau >= SOS_PD * SB) {
            float4 xs[SOS_PD][NL];
#pragma unroll
            for (int u = 0; u < SOS_PD; ++u) ld(xs[u], tau + u * SB);
            for (; tau + 2 * SOS_PD * SB <= limit; tau += SOS_PD * SB) {
#pragma unroll
                for (int u = 0; u < SOS_PD; ++u) {
                    run(xs[u], tau + u * SB, store);
                    __builtin_amdgcn_sched_barrier(0);
                    ld(xs[u], tau + (u + SOS_PD) * SB);
                }
            }
#pragma unroll
            for (int u = 0; u < SOS_PD; ++u) run(xs[u], tau + u * SB, store);
            tau += SOS_PD * SB;
        }
    }
    for (; tau < hi + 3; ++tau) tick(tau);
}

template <bool FWD, int QT>
__device__ __forceinline__ void tl_tile(const float *xr, int comp, float *sp, float *op, size_t so, const TlGeo &G,
                                        int sec, bool own, Biquad<float> &bq, long a, long lo, long hi, float2 &S,
                                        float2 &E) {
    if constexpr (FWD) tl_fwd_tile(xr, comp, G.N, sp, sec, own, bq, a, lo, hi, S, E);
    else tl_bwd_tile<QT>(sp, G.N, G.L, op, so, sec, own, bq, a, lo, hi, S, E);
}

__device__ __forceinline__ Biquad<float> tl_section(const float *sos, int s, float z0, float z1) {
    return Biquad<float>{sos[6 * s], sos[6 * s + 1], sos[6 * s + 2], sos[6 * s + 4], sos[6 * s + 5], z0, z1};
}

// Step 1.  Virtual stream v = k * 2C + g in BankLane's lane mapping (tile-major: the 16 virtual
// streams of a wave are tiles of about the same length); tail lanes shadow the last one and store
// nothing.  Sst / Est: [2C][K][4 sections] float2.
template <bool FWD, int QT>
__global__ __launch_bounds__(256) void k_tl_spec(const float *__restrict__ x, float *__restrict__ scr,
                                                 float *__restrict__ out, Lay lo_, TlGeo G,
                                                 const float *__restrict__ sos, const float *__restrict__ zi,
                                                 float2 *__restrict__ Sst, float2 *__restrict__ Est) {
    const int lane = threadIdx.x & 63, w = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int sec = (lane >> 2) & 3;
    const int v = 16 * w + 4 * (lane >> 4) + (lane & 3), nv = 2 * G.C * G.K;
    const bool own = v < nv;
    const int vv = min(v, nv - 1), k = vv / (2 * G.C), g = vv % (2 * G.C);
    const int ch = g >> 1, comp = g & 1;
    const float *xr = x + (size_t)ch * G.N * 2;
    float *sp = scr + (size_t)g * G.Lp;
    float *op = out + lo_.off(ch, 0) + comp;
    const long lo = (long)k * G.T, hi = lmin(lo + G.T, G.L), a = lmax(0, lo - G.W);
    float z0 = 0, z1 = 0;
    if (a == 0) {   // the pass's own start: sosfilt_zi * first sample, as the sequential kernels set it
        const float x0 = FWD ? tl_ext(xr, comp, G.N, 0) : sp[G.L - 1];
        z0 = zi[2 * sec] * x0;
        z1 = zi[2 * sec + 1] * x0;
    }
    Biquad<float> bq = tl_section(sos, sec, z0, z1);
    float2 S = make_float2(0, 0), E = S;
    tl_tile<FWD, QT>(xr, comp, sp, op, lo_.s_n, G, sec, own, bq, a, lo, hi, S, E);
    if (own) {
        const size_t i = ((size_t)g * G.K + k) * 4 + sec;
        Sst[i] = S;
        Est[i] = E;
    }
}

// Step 2.  One stream per lane quad (BankLane); stats[0] += tiles checked, stats[1] += tiles rerun.
template <bool FWD, int QT>
__global__ __launch_bounds__(256) void k_tl_resolve(const float *__restrict__ x, float *__restrict__ scr,
                                                    float *__restrict__ out, Lay lo_, TlGeo G,
                                                    const float *__restrict__ sos, const float2 *__restrict__ Sst,
                                                    const float2 *__restrict__ Est, int32_t *__restrict__ stats) {
    const BankLane bl(G.C);
    const int sec = bl.sec, g = 2 * bl.ch + bl.comp;
    const float *xr = x + (size_t)bl.ch * G.N * 2;
    float *sp = scr + (size_t)g * G.Lp;
    float *op = out + lo_.off(bl.ch, 0) + bl.comp;
    const float2 *Sg = Sst + (size_t)g * G.K * 4 + sec, *Eg = Est + (size_t)g * G.K * 4 + sec;
    float2 e = Eg[0];
    int rerun = 0;
    for (int k = 1; k < G.K; ++k) {
        const float2 s = Sg[4 * k];
        int same = __float_as_uint(s.x) == __float_as_uint(e.x) && __float_as_uint(s.y) == __float_as_uint(e.y);
        same &= __shfl_xor(same, 4);   // over the stream's four section lanes
        same &= __shfl_xor(same, 8);
        if (same) {
            e = Eg[4 * k];
        } else {
            ++rerun;
            const long lo = (long)k * G.T, hi = lmin(lo + G.T, G.L);
            Biquad<float> bq = tl_section(sos, sec, e.x, e.y);
            float2 S = make_float2(0, 0);
            tl_tile<FWD, QT>(xr, bl.comp, sp, op, lo_.s_n, G, sec, bl.own, bq, lo, lo, hi, S, e);
        }
    }
    if (bl.own && sec == 0) {
        atomicAdd(stats, G.K - 1);
        if (rerun) atomicAdd(stats + 1, rerun);
    }
}

template <int QT>
void tl_launch(tetra_ctx *ctx, const float *x, float *scr, float *out, Lay lo, const TlGeo &G, const float *coef,
               float2 *Sst, float2 *Est, int32_t *stats) {
    const unsigned blk = 256;
    const dim3 gs(grid_for((size_t)8 * G.C * G.K, blk)), gr(grid_for((size_t)8 * G.C, blk));
    {
        PROF(ctx, "compat_tiled_fwd");
        hipLaunchKernelGGL((k_tl_spec<true, 0>), gs, dim3(blk), 0, ctx->stream, x, scr, out, lo, G, coef, coef + 24, Sst,
                           Est);
        hipLaunchKernelGGL((k_tl_resolve<true, 0>), gr, dim3(blk), 0, ctx->stream, x, scr, out, lo, G, coef,
                           (const float2 *)Sst, (const float2 *)Est, stats);
    }
    {
        PROF(ctx, "compat_tiled_bwd");
        hipLaunchKernelGGL((k_tl_spec<false, QT>), gs, dim3(blk), 0, ctx->stream, x, scr, out, lo, G, coef, coef + 24, Sst,
                           Est);
        hipLaunchKernelGGL((k_tl_resolve<false, QT>), gr, dim3(blk), 0, ctx->stream, x, scr, out, lo, G, coef,
                           (const float2 *)Sst, (const float2 *)Est, stats + 2);
    }
}

}  // namespace

bool tiled_fits(const tetra_compat_plan *P, size_t C, size_t N, int tile) {
    if (tile <= 0) tile = TL_TILE;
    return P->dec_f64 == 0 && C >= 1 && C <= (size_t)TL_MAXC && P->q >= 7 && P->q <= 10 && N > (size_t)tile &&
           N < ((size_t)1 << 30) && (N + 2 * TL_PAD) / (size_t)tile < TL_MAXK;
}

int run_decimate_tiled(tetra_ctx *ctx, const tetra_compat_plan *P, const float *x, int C, long N, float *out,
                       size_t s_grp, size_t s_n, size_t s_lane) {
    const Lay lo{s_grp, s_n, s_lane};
    const long L = N + 2 * TL_PAD;
    const long Lp = (L + 3) & ~3L;
    const int T = ctx->tl_tile > 0 ? ctx->tl_tile : TL_TILE, W = ctx->tl_warm > 0 ? ctx->tl_warm : TL_WARM;
    const TlGeo G{C, (int)ceil_div(L, T), T, W, N, L, Lp};
    const size_t nst = (size_t)2 * C * G.K * 4;   // float2 state words per array
    float *scr = (float *)ws(ctx, S_W0, (size_t)2 * C * Lp * sizeof(float));
    float *coef = (float *)ws(ctx, S_W7, 32 * sizeof(float));
    char *tl = (char *)ws(ctx, S_W20, 16 + 2 * nst * sizeof(float2));
    if (!scr || !coef || !tl) return TETRA_E_NOMEM;
    int32_t *stats = (int32_t *)tl;
    float2 *Sst = (float2 *)(tl + 16), *Est = Sst + nst;
    const int rc = upload_sos_coef(ctx, P, coef);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(stats, 0, 16, ctx->stream));
    switch (P->q) {
        case 7: tl_launch<7>(ctx, x, scr, out, lo, G, coef, Sst, Est, stats); break;
        case 8: tl_launch<8>(ctx, x, scr, out, lo, G, coef, Sst, Est, stats); break;
        case 9: tl_launch<9>(ctx, x, scr, out, lo, G, coef, Sst, Est, stats); break;
        case 10: tl_launch<10>(ctx, x, scr, out, lo, G, coef, Sst, Est, stats); break;
        default: return tetra_fail(ctx, TETRA_E_INVALID, "tiled decimator: q %d outside 7..10", P->q);
    }
    HIP_TRY(ctx, hipGetLastError());
    ctx->tl_ran = true;
    return TETRA_OK;
}

extern "C" {

int tetra_compat_set_tiles(tetra_ctx *ctx, int tile, int warm) {
    if (!ctx) return TETRA_E_INVALID;
    if (tile == 0 && warm == 0) {
        ctx->tl_tile = ctx->tl_warm = 0;
        return TETRA_OK;
    }
    if (tile < 64 || warm < 64 || tile % 64 || warm % 64 || tile > (1 << 24) || warm > (1 << 24))
        return tetra_fail(ctx, TETRA_E_INVALID, "tile and warm-up lengths are multiples of 64, >= 64 (or 0, 0)");
    ctx->tl_tile = tile;
    ctx->tl_warm = warm;
    return TETRA_OK;
}

int tetra_compat_tile_stats(tetra_ctx *ctx, int32_t *stats) {
    if (!ctx || !stats) return TETRA_E_INVALID;
    std::memset(stats, 0, 4 * sizeof(int32_t));
    if (!ctx->tl_ran || !ctx->slot[S_W20].p) return TETRA_OK;
    HIP_TRY(ctx, hipMemcpyAsync(stats, ctx->slot[S_W20].p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TETRA_OK;
}

int tetra_decimate_tiled(tetra_ctx *ctx, const tetra_compat_plan *P, const void *iq, int fmt, size_t C, size_t N,
                         void *out) {
    if (!ctx) return TETRA_E_INVALID;
    if (!P || fmt != TETRA_CF32 || !tiled_fits(P, C, N, ctx->tl_tile)) {
        ctx->tl_ran = false;
        return tetra_decimate(ctx, P, iq, fmt, C, N, out);   // the sequential kernels: exact either way
    }
    const size_t M = (size_t)ceil_div((long)N, P->q);
    Staging st(ctx);
    const void *x = st.in(iq, C * N * 8);
    void *o = st.out(out, C * M * 8);
    if (!x || !o) return st.finish();
    const Lay lo = row_major((long)M);
    const int rc = run_decimate_tiled(ctx, P, (const float *)x, (int)C, (long)N, (float *)o, lo.s_grp, lo.s_n, lo.s_lane);
    if (rc) return rc;
    return st.finish();
}

}  // extern "C"
