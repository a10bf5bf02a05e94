// compat_decimate.hip -- stage 1 of the compat chain (compat_demod.hip: numerics, layouts):
// scipy.signal.decimate(x, q), sequential in time or, opt-in, time-blocked (time-tiled: compat_tiled.hip).
#include "common.h"
#include "compat_sos.h"   // Lay, Biquad, the banked lane mapping: shared with compat_tiled.hip

namespace {

// ------------------------------------------------------------------ decimator (sosfiltfilt)
// Skewed section pipeline: lane = (channel, component, section).  The 4 sections of one stream sit
// in 4 adjacent lanes; at tick tau section s processes ext sample tau - s, and its input is the
// output section s-1 produced at tick tau-1 (one DPP row shift).  Each lane runs one biquad per
// tick, so a stream's 36-operation step becomes a 9-operation tick on 4x the lanes -- the
// arithmetic (scipy _sosfilt's operation order per section and sample) is unchanged.
template <typename T>
__device__ __forceinline__ T from_left(T v) {   // lane l receives v of lane l-1 (row shift, DPP)
    if constexpr (sizeof(T) == 4) {
        return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));
    } else {
        const long long b = __builtin_bit_cast(long long, v);
        const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffff), 0x111, 0xf, 0xf, true);
        const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x111, 0xf, 0xf, true);
        return __builtin_bit_cast(T, ((long long)hi << 32) | (unsigned int)lo);
    }
}

constexpr int SKB = 32;   // ticks per prefetch batch (a multiple of every vector width below)

// 16-byte vectors: the decimator's memory traffic goes through as few VMEM instructions as
// possible -- with one wave per SIMD the per-wave limit on outstanding VMEM operations, not
// bandwidth or arithmetic, sets the tick rate when every tick loads and stores.
template <typename T> struct Vec16;
template <> struct Vec16<float> { using type = float4; static constexpr int n = 4; };
template <> struct Vec16<double> { using type = double2; static constexpr int n = 2; };
template <typename V> __device__ __forceinline__ auto velt(const V &v, int i) {   // i compile-time after unroll
    if constexpr (sizeof(V) == 4 * sizeof(v.x)) return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
    else return i == 0 ? v.x : v.y;
}

// Forward pass over the odd extension ext[0, L) of one stream, L = N + 2 pad.  Scratch is
// stream-major: stream g = 2 ch + comp at scr[g * Lp + j] (Lp a multiple of 4), so a lane's
// consecutive outputs are one vector store.  Input rows are complex [C][N]; a vector load holds
// CPV consecutive complex samples of both components (CPV = 2 for complex64 rows of even length).
template <typename T, int CPV>
__global__ __launch_bounds__(256) void k_sos_fwd(const T *__restrict__ x, int C, long N, int pad,
                                                const T *__restrict__ sos, const T *__restrict__ zi,
                                                T *__restrict__ scr, long Lp) {
    using V = typename Vec16<T>::type;
    constexpr int VW = Vec16<T>::n;           // outputs per vector store
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int g = gid >> 2, sec = gid & 3;
    const int ch = min(g >> 1, C - 1), comp = g & 1;   // tail lanes shadow the last stream, store nothing
    const bool own = (g >> 1) < C;
    const bool st = own && sec == 3;
    const T *xr = x + (size_t)ch * N * 2;      // complex row
    const long L = N + 2 * pad;
    auto xat = [&](long n) { return xr[2 * n + comp]; };
    const T two = 2, x0 = xat(0), xl = xat(N - 1);
    auto ext = [&](long j) -> T {   // scipy _arraytools.odd_ext
        if (j < pad) return two * x0 - xat(pad - j);
        if (j < pad + N) return xat(j - pad);
        return two * xl - xat(N - 2 - (j - pad - N));
    };
    Biquad<T> bq = load_section(sos, zi, sec, ext(0));
    T *sp = scr + (size_t)(2 * ch + comp) * Lp;
    T y = 0;
    auto tick = [&](long tau, T xin) __attribute__((always_inline)) {
        const T left = from_left(y);
        const long j = tau - sec;
        if (j >= 0 && j < L) {
            y = bq.step(sec == 0 ? xin : left);
            if (st) sp[j] = y;
        }
    };
    long tau = 0;
    for (; tau < pad; ++tau) tick(tau, ext(tau));
    // body: section 0 reads x[tau - pad] (vector loads of CPV complex samples, double-buffered one
    // batch ahead); section 3 emits j = tau - 3, aligned to VW because pad - 3 = 24.
    using PV = typename std::conditional<CPV * 2 * sizeof(T) == 16, V,
                                         typename std::conditional<sizeof(T) == 4, float2, double2>::type>::type;
    constexpr int NL = SKB / CPV;              // input vectors per batch
    PV xa[NL], xb[NL];
    auto ld = [&](PV (&v)[NL], long t0) __attribute__((always_inline)) {
        const PV *src = reinterpret_cast<const PV *>(xr + 2 * (t0 - pad));
#pragma unroll
        for (int k = 0; k < NL; ++k) v[k] = src[k];
    };
    auto run = [&](PV (&v)[NL], long t0) __attribute__((always_inline)) {
        T o[VW];
#pragma unroll
        for (int u = 0; u < SKB; ++u) {
            const PV &pv = v[u / CPV];
            const T xin = velt(pv, 2 * (u % CPV) + comp);
            const T left = from_left(y);
            y = bq.step(sec == 0 ? xin : left);   // all sections active: pad >= 3
            o[u % VW] = y;
            if (u % VW == VW - 1) {
                V w;
                if constexpr (VW == 4) w = V{o[0], o[1], o[2], o[3]};
                else w = V{o[0], o[1]};
                if (st) *reinterpret_cast<V *>(sp + (t0 + u - 3 - (VW - 1))) = w;   // section-3 lanes only
            }
        }
    };
    if (N >= 2 * SKB) {
        ld(xa, tau);
        ld(xb, tau + SKB);
        for (; tau + 4 * SKB <= pad + N; tau += 2 * SKB) {
            run(xa, tau);
            __builtin_amdgcn_sched_barrier(0);
            ld(xa, tau + 2 * SKB);
            run(xb, tau + SKB);
            __builtin_amdgcn_sched_barrier(0);
            ld(xb, tau + 3 * SKB);
        }
        run(xa, tau);
        run(xb, tau + SKB);
        tau += 2 * SKB;
    }
    for (; tau < L + 3; ++tau) tick(tau, tau < L ? ext(tau) : T(0));
}

// Reverse pass (sosfiltfilt's second sosfilt over the time-reversed forward output), keeping
// decimate's y[::q]: output t (= ext index t + pad) when t % q == 0.
template <typename T, int QT>
__global__ __launch_bounds__(256) void k_sos_bwd(const T *__restrict__ scr, long Lp, int C, long N, int pad, int q,
                                                const T *__restrict__ sos, const T *__restrict__ zi,
                                                T *__restrict__ out, Lay lo) {
    using V = typename Vec16<T>::type;
    constexpr int VW = Vec16<T>::n;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int g = gid >> 2, sec = gid & 3;
    const int ch = min(g >> 1, C - 1), comp = g & 1;
    const bool own = (g >> 1) < C;
    const T *sp = scr + (size_t)(2 * ch + comp) * Lp;
    const long L = N + 2 * pad;
    Biquad<T> bq = load_section(sos, zi, sec, sp[L - 1]);
    T *op = out + lo.off(ch, 0) + comp;
    const size_t so = lo.s_n;
    const bool st = own && sec == 3;
    T y = 0;
    // tick tau: section 0 reads scr[L-1-tau]; section s works on ext index j = L-1-(tau-s)
    auto tick = [&](long tau, T xin) __attribute__((always_inline)) {
        const T left = from_left(y);
        const long k = tau - sec;
        if (k >= 0 && k < L) {
            y = bq.step(sec == 0 ? xin : left);
            const int t = (int)(L - 1 - k - pad);
            if (st && t >= 0 && t < N && t % q == 0) op[(size_t)(t / q) * so] = y;
        }
    };
    long tau = 0;
    if constexpr (QT == 0) {
        // body batches start where the first vector load is aligned: (L - tau) % VW == 0, tau >= 3
        long tau0 = 3;
        while ((L - tau0) % VW) ++tau0;
        for (; tau < tau0; ++tau) tick(tau, sp[L - 1 - tau]);
        constexpr int NL = SKB / VW;
        V xa[NL], xb[NL];
        auto ld = [&](V (&v)[NL], long t0) __attribute__((always_inline)) {
            // ticks t0 .. t0+SKB-1 read j = L-1-t0 down to L-t0-SKB; vector k covers
            // [L - t0 - (k+1) VW, L - t0 - k VW)
    #pragma unroll
            for (int k = 0; k < NL; ++k) v[k] = *reinterpret_cast<const V *>(sp + (L - t0 - (k + 1) * VW));
        };
        // The output lanes' index t = L-1-(tau-3)-pad falls by one per tick and is the same for every
        // stream (equal lengths), so t / q and t % q are wave-uniform scalars: the decimating store is
        // a scalar branch, not per-lane arithmetic.
        int tc = 0, tq = 0, tr = 0;
        auto run = [&](V (&v)[NL], long t0) __attribute__((always_inline)) {
    #pragma unroll
            for (int u = 0; u < SKB; ++u) {
                const T xin = velt(v[u / VW], VW - 1 - (u % VW));
                const T left = from_left(y);
                y = bq.step(sec == 0 ? xin : left);
                if (tr == 0 && tc >= 0 && tc < N) {
                    if (st) op[(size_t)tq * so] = y;
                }
                --tc;
                if (--tr < 0) { tr = q - 1; --tq; }
            }
        };
        if (L - tau >= 2 * SKB) {
            tc = __builtin_amdgcn_readfirstlane((int)(L - 1 - (tau - 3) - pad));   // >= 0 here
            tq = __builtin_amdgcn_readfirstlane(tc / q);
            tr = __builtin_amdgcn_readfirstlane(tc % q);
            ld(xa, tau);
            ld(xb, tau + SKB);
            for (; tau + 4 * SKB <= L; tau += 2 * SKB) {
                run(xa, tau);
                __builtin_amdgcn_sched_barrier(0);
                ld(xa, tau + 2 * SKB);
                run(xb, tau + SKB);
                __builtin_amdgcn_sched_barrier(0);
                ld(xb, tau + 3 * SKB);
            }
            run(xa, tau);
            run(xb, tau + SKB);
            tau += 2 * SKB;
        }
    } else {
        // q = QT known at compile time: batches of SB ticks (a multiple of QT and of VW) that start
        // where the vector load is aligned, inside the span where every output index lies in [0, N).
        // The output phase ph (the first tick u of a batch with t % QT == 0) is then the same for
        // every batch (it cannot always be 0: with the odd pad the aligned starts have odd t), so
        // the section output of each tick goes to a register yr[u] and the batch ends with SB / QT
        // stores of yr[ph + k QT] -- no per-tick counters or branches.
        constexpr int SB = (2 * QT) % VW == 0 ? 2 * QT : 4 * QT;
        constexpr int NL = SB / VW;
        auto tcur = [&](long tt) { return L - 1 - (tt - 3) - pad; };   // output index t of section 3 at tick tt
        long tau0 = pad + 3;   // first tick whose t < N
        while ((L - tau0) % VW) ++tau0;
        const int ph = __builtin_amdgcn_readfirstlane((int)(tcur(tau0) % QT));   // t % QT == 0 at u = ph
        for (; tau < tau0; ++tau) tick(tau, sp[L - 1 - tau]);
        V xa[NL], xb[NL];
        auto ld = [&](V (&v)[NL], long t0) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < NL; ++k) v[k] = *reinterpret_cast<const V *>(sp + (L - t0 - (k + 1) * VW));
        };
        T *dst0 = op;
        auto run = [&](V (&v)[NL], long t0) __attribute__((always_inline)) {
            const long tq0 = (tcur(t0) - ph) / QT;   // wave-uniform: output index of tick ph
            T yr[SB];
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const T xin = velt(v[u / VW], VW - 1 - (u % VW));
                const T left = from_left(y);
                y = bq.step(sec == 0 ? xin : left);
                yr[u] = y;
            }
            if (st) {
#pragma unroll
                for (int k = 0; k < SB / QT; ++k) dst0[(size_t)(tq0 - k) * so] = yr[ph + k * QT];
            }
        };
        // batches while the last tick of the next two batches still has t >= 0 (t = tcur(tau + 2 SB - 1))
        if (tcur(tau + 2 * SB - 1) >= 0 && L - tau >= 2 * SB) {
            ld(xa, tau);
            ld(xb, tau + SB);
            for (; tcur(tau + 4 * SB - 1) >= 0 && tau + 4 * SB <= L; tau += 2 * SB) {
                run(xa, tau);
                __builtin_amdgcn_sched_barrier(0);
                ld(xa, tau + 2 * SB);
                run(xb, tau + SB);
                __builtin_amdgcn_sched_barrier(0);
                ld(xb, tau + 3 * SB);
            }
            run(xa, tau);
            run(xb, tau + SB);
            tau += 2 * SB;
        }
    }
    for (; tau < L + 3; ++tau) tick(tau, tau < L ? sp[L - 1 - tau] : T(0));
}

// ------------------------------------------------------------------ fp32 decimator, banked lanes
// (the lane mapping and its DPP moves: compat_sos.h)
// Forward pass (k_sos_fwd's contract) for complex64 rows of any length: the window loads are
// 4-byte-aligned vectors (f4u), so an odd-length row's 8-byte-aligned start is fine, and the
// batches stop one sample short of the row end (below).  Window of 8 samples:
// lane (sec = j) loads floats [2 n0 + 4 j + comp, +4): elements 0 and 2 are component `comp` of
// samples n0 + 2j and n0 + 2j + 1.
__global__ __launch_bounds__(256) void k_sos_fwd_bank(const float *__restrict__ x, int C, long N, int pad,
                                                     const float *__restrict__ sos, const float *__restrict__ zi,
                                                     float *__restrict__ scr, long Lp) {
    const BankLane bl(C);
    const int sec = bl.sec, comp = bl.comp;
    const bool st = bl.st;
    const float *xr = x + (size_t)bl.ch * N * 2;
    const long L = N + 2 * pad;
    auto xat = [&](long n) { return xr[2 * n + comp]; };
    const float two = 2, x0 = xat(0), xl = xat(N - 1);
    auto ext = [&](long j) -> float {   // scipy _arraytools.odd_ext
        if (j < pad) return two * x0 - xat(pad - j);
        if (j < pad + N) return xat(j - pad);
        return two * xl - xat(N - 2 - (j - pad - N));
    };
    Biquad<float> bq = load_section(sos, zi, sec, ext(0));
    float *sp = scr + (size_t)(2 * bl.ch + comp) * Lp;
    float y = 0;
    auto tick = [&](long tau, float xin) __attribute__((always_inline)) {
        const float left = from_left_bank(y);
        const long j = tau - sec;
        if (j >= 0 && j < L) {
            y = bq.step(sec == 0 ? xin : left);
            if (st) sp[j] = y;
        }
    };
    long tau = 0;
    for (; tau < pad; ++tau) tick(tau, ext(tau));
    constexpr int NW = SKB / 8;   // 8-sample windows per batch
    const float *xw = xr + 4 * sec + comp;
    auto ld = [&](f4u (&v)[NW], long t0) __attribute__((always_inline)) {
        const float *src = xw + 2 * (t0 - pad);
#pragma unroll
        for (int k = 0; k < NW; ++k) v[k] = *reinterpret_cast<const f4u *>(src + 16 * k);
    };
    // Output: section 3 emits j = tau - 3.  Every 16 ticks the four lanes of a stream each store 4
    // of section 3's last 16 outputs (bank j takes o[4j .. 4j+3] from bank 3 with row_shl:4(3-j)):
    // one 64-lane store of 64 contiguous bytes per stream instead of four 16-lane stores of 16.
    const bool own = bl.own;
    auto run = [&](f4u (&v)[NW], long t0) __attribute__((always_inline)) {
        float o[16];
#pragma unroll
        for (int u = 0; u < SKB; ++u) {
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
            y = bq.step(xin);   // every section active: pad >= 3
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
                if (own) *reinterpret_cast<float4 *>(sp + (t0 + u - 18 + 4 * sec)) = float4{w[0], w[1], w[2], w[3]};
            }
        }
        // elements 1 and 3 are never read: keep the whole vector live to here, or the allocator
        // reuses them as temporaries while the next window's load into them is in flight (a
        // write-after-write wait on every outstanding load)
#pragma unroll
        for (int k = 0; k < NW; ++k) asm volatile("" ::"v"(v[k]));
    };
    // the imaginary lanes of the last chunk read one float past their window: the batches stop
    // one sample short of the row end, so that float is inside the row.  SOS_PD batches in flight.
    if (N >= SOS_PD * SKB + 1) {
        f4u xs[SOS_PD][NW];
#pragma unroll
        for (int u = 0; u < SOS_PD; ++u) ld(xs[u], tau + u * SKB);
        for (; tau + 2 * SOS_PD * SKB < pad + N; tau += SOS_PD * SKB) {
#pragma unroll
            for (int u = 0; u < SOS_PD; ++u) {
                run(xs[u], tau + u * SKB);
                __builtin_amdgcn_sched_barrier(0);
                ld(xs[u], tau + (u + SOS_PD) * SKB);
            }
        }
#pragma unroll
        for (int u = 0; u < SOS_PD; ++u) run(xs[u], tau + u * SKB);
        tau += SOS_PD * SKB;
    }
    for (; tau < L + 3; ++tau) tick(tau, tau < L ? ext(tau) : 0.f);
}

// Reverse pass with decimation q = QT (k_sos_bwd<float, QT>'s contract).  The scratch row is the
// stream's own, so the 4 lanes of a stream load the 4 chunks of a 16-tick window with no
// duplication: lane (sec = j) loads floats [L - t0 - 16 k - 4 j - 4, +4), tick u of the window reads
// element 3 - (u & 3) of chunk (u >> 2) & 3.  The batch start is chosen so that the first output
// tick of every batch is the compile-time phase PH, so outputs are stored as they are produced.
template <int QT>
__global__ __launch_bounds__(256) void k_sos_bwd_bank(const float *__restrict__ scr, long Lp, int C, long N, int pad,
                                                     int q, const float *__restrict__ sos,
                                                     const float *__restrict__ zi, float *__restrict__ out, Lay lo) {
    const BankLane bl(C);
    const int sec = bl.sec;
    const bool st = bl.st;
    const float *sp = scr + (size_t)(2 * bl.ch + bl.comp) * Lp;
    const long L = N + 2 * pad;
    Biquad<float> bq = load_section(sos, zi, sec, sp[L - 1]);
    float *op = out + lo.off(bl.ch, 0) + bl.comp;
    const size_t so = lo.s_n;
    float y = 0;
    auto tick = [&](long tau, float xin) __attribute__((always_inline)) {
        const float left = from_left_bank(y);
        const long k = tau - sec;
        if (k >= 0 && k < L) {
            y = bq.step(sec == 0 ? xin : left);
            const int t = (int)(L - 1 - k - pad);
            if (st && t >= 0 && t < N && t % q == 0) op[(size_t)(t / q) * so] = y;
        }
    };
    constexpr int SB = QT * 16 / (QT % 16 == 0 ? 16 : QT % 8 == 0 ? 8 : QT % 4 == 0 ? 4 : QT % 2 == 0 ? 2 : 1);
    static_assert(SB % 16 == 0 && SB % QT == 0, "batch = lcm(16, QT)");
    constexpr int NL = SB / 16;
    // output index of section 3 at tick tt; t % QT == 0 at tick u of a batch iff u % QT == PH
    auto tcur = [&](long tt) { return L - 1 - (tt - 3) - pad; };
    // PH must match the parity that the aligned starts allow (tcur(tau0) = L - tau0 + 2 - pad with
    // L - tau0 a multiple of 4): odd for even QT and the default odd pad
    constexpr int PH = QT % 2 ? 0 : 5 % QT;
    long tau0 = pad + 3;
    while (((L - tau0) % 4 || tcur(tau0) % QT != PH) && tau0 < pad + 3 + 4 * QT) ++tau0;
    const bool phased = (L - tau0) % 4 == 0 && tcur(tau0) % QT == PH;
    long tau = 0;
    if (phased) {
        for (; tau < tau0; ++tau) tick(tau, sp[L - 1 - tau]);
        const float *sw = sp + L - 4 - 4 * sec;
        auto ld = [&](float4 (&v)[NL], long t0) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < NL; ++k) v[k] = *reinterpret_cast<const float4 *>(sw - t0 - 16 * k);
        };
        auto run = [&](float4 (&v)[NL], long t0) __attribute__((always_inline)) {
            const long tq0 = tcur(t0 + PH) / QT;   // wave-uniform: output index of tick PH
#pragma unroll
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
                if (u % QT == PH && st) op[(size_t)(tq0 - u / QT) * so] = y;
            }
        };
        if (tcur(tau + SOS_PD * SB - 1) >= 0 && L - tau >= SOS_PD * SB) {
            float4 xs[SOS_PD][NL];
#pragma unroll
            for (int u = 0; u < SOS_PD; ++u) ld(xs[u], tau + u * SB);
            for (; tcur(tau + 2 * SOS_PD * SB - 1) >= 0 && tau + 2 * SOS_PD * SB <= L; tau += SOS_PD * SB) {
#pragma unroll
                for (int u = 0; u < SOS_PD; ++u) {
                    run(xs[u], tau + u * SB);
                    __builtin_amdgcn_sched_barrier(0);
                    ld(xs[u], tau + (u + SOS_PD) * SB);
                }
            }
#pragma unroll
            for (int u = 0; u < SOS_PD; ++u) run(xs[u], tau + u * SB);
            tau += SOS_PD * SB;
        }
    }
    for (; tau < L + 3; ++tau) tick(tau, tau < L ? sp[L - 1 - tau] : 0.f);
}

// ------------------------------------------------------------------ time-blocked decimator (latency mode)
// sosfiltfilt for a few channels, parallel in time.  A stream's
// odd extension ext[0, L) is cut into tiles of SB_B samples; one quad of lanes runs the 4-section
// cascade over one tile (the skewed section pipeline of k_sos_fwd: section s works on sample tau - s
// at tick tau), so every tile of every stream recurses at once.  Per pass (forward, then backward on
// the reversed forward output):
//   1. k_sosb_tile<.., false>: each tile from zero state -> its end state e_k (8 numbers: the two
//      DF-II-T states of 4 sections), T arithmetic;
//   2. k_sosb_scan: the true start states s_k of every tile in float64, s_{k+1} = Phi s_k + e_k with
//      Phi = A^SB_B (A: the cascade's one-sample zero-input transition), s_0 = sosfilt_zi * ext[0] as
//      the sequential pass sets it -- as an inclusive Hillis-Steele scan over the tiles with the
//      host's table Phi^(2^r) (compat_blocked_table);
//   3. k_sosb_tile<.., true>: each tile again from (T) s_k, its outputs to the scratch row (forward)
//      or decimated to `out` (backward).
// Tile 0 starts from the sequential pass's exact state, so its outputs are scipy's bit for bit;
// later tiles start from the float64-composed state instead of the state a sequential fp32
// recursion would have accumulated, so outputs differ from scipy's by the filter's fp32 noise
// (measured on the 31 reference fixtures: <= 3.4e-6 on .symbols for q <= 10, no hard decision
// changed; oracle/compat.py: decimate_blocked restates every operation and the GPU equals it bit
// for bit).  Used by tetra_demod_compat for C <= SB_MAXC channels and q <= SB_MAXQ (at q = 83 the
// cheby1 band is so narrow the noise reaches 5.7e-5), and never by the component entry point
// tetra_decimate, which stays scipy-exact.
// stream-tiles per workgroup: few, so one channel's tiles spread over many CUs; SB_LT threads stage
// them (SB_B ST / SB_LT loads each), wave 0's 4 ST lanes run the recursion
template <typename T> struct SbCfg { static constexpr int ST = 16; };
constexpr int SB_LT = 256;

struct SbGeo {
    int C, Tn, pad, q;
    long N, L, Lp;
};

// stream-tile g = (ch * Tn + tile) * 2 + comp
template <typename T, bool FWD, bool FINAL>
__global__ __launch_bounds__(SB_LT) void k_sosb_tile(const T *__restrict__ x, T *__restrict__ scr, SbGeo G,
                                                                const T *__restrict__ sos,
                                                                const double *__restrict__ states,
                                                                double *__restrict__ ends, T *__restrict__ out, Lay lo) {
    constexpr int ST = SbCfg<T>::ST;
    __shared__ T buf[ST][SB_B + 1];
    __shared__ int rch[ST], rtile[ST];   // the rows' channel and tile: one division per row, not per element
    const int tid = threadIdx.x, sec = tid & 3, stl = tid >> 2;
    const long ntiles = (long)2 * G.C * G.Tn;
    const int nrow = (int)min((long)ST, ntiles - (long)blockIdx.x * ST);   // rows this workgroup owns
    if (tid < ST) {
        const int pr = (int)((((long)blockIdx.x * ST + (tid < nrow ? tid : 0))) >> 1);
        rtile[tid] = pr % G.Tn;
        rch[tid] = pr / G.Tn;
    }
    __syncthreads();
    // cooperative load of the workgroup's tiles: ext (forward) or the reversed scratch row (backward).
    // A single channel is a few workgroups, so each thread's 64 loads are what the pass waits for:
    // they go out 16 at a time (unconditional, from clamped indices), and ext's odd-extension
    // arithmetic at the row ends is applied afterwards to the raw samples it reflects.
    constexpr int PER = ST * SB_B / SB_LT, U = PER < 16 ? PER : 16;
    static_assert(PER % U == 0 && 4 * ST <= 64, "loads per thread; the recursion fits wave 0");
    auto src = [&](int i, int &r, int &j, long &e, int &ch, int &comp, bool &in) -> const T * {
        r = i / SB_B;
        j = i % SB_B;
        in = r < nrow;
        const int rr = in ? r : 0;
        comp = rr & 1;   // ST is even: row parity = stream-tile parity
        const int tile = rtile[rr];
        ch = rch[rr];
        e = (long)tile * SB_B + j;
        in = in && e < G.L;
        const long ec = in ? e : 0;
        if (FWD) {   // the sample scipy's odd_ext reflects (or copies) at ext index e
            const long n = ec < G.pad ? G.pad - ec : (ec < G.pad + G.N ? ec - G.pad : G.N - 2 - (ec - G.pad - G.N));
            return x + (size_t)ch * G.N * 2 + comp + 2 * n;
        }
        return scr + (size_t)(2 * ch + comp) * G.Lp + (G.L - 1 - ec);
    };
    for (int c0 = 0; c0 < PER; c0 += U) {
        T v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int r, j, ch, comp;
            long e;
            bool in;
            v[u] = *src(tid + SB_LT * (c0 + u), r, j, e, ch, comp, in);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int r, j, ch, comp;
            long e;
            bool in;
            src(tid + SB_LT * (c0 + u), r, j, e, ch, comp, in);
            T w = in ? v[u] : (T)0;
            if (FWD && in && (e < G.pad || e >= G.pad + G.N)) {   // scipy _arraytools.odd_ext, in T
                const T *xr = x + (size_t)ch * G.N * 2 + comp;
                w = (T)2 * (e < G.pad ? xr[0] : xr[2 * (G.N - 1)]) - w;
            }
            buf[r][j] = w;
        }
    }
    __syncthreads();
    if (tid < 4 * ST) {   // wave 0: the recursion (wave-uniform branch)
    const long g = (long)blockIdx.x * ST + stl;
    const bool own = g < ntiles;
    const int tile = own ? (int)((g >> 1) % G.Tn) : 0;
    const long len = own ? min((long)SB_B, G.L - (long)tile * SB_B) : 0;
    Biquad<T> bq{sos[6 * sec], sos[6 * sec + 1], sos[6 * sec + 2], sos[6 * sec + 4], sos[6 * sec + 5], (T)0, (T)0};
    if (FINAL && own) {
        bq.z0 = (T)states[g * 8 + 2 * sec];
        bq.z1 = (T)states[g * 8 + 2 * sec + 1];
    }
    // Ticks 0-2 and SB_B..SB_B+2 are guarded (a section starts at tick sec and ends at SB_B - 1 + sec);
    // the rest are branch-free: every lane steps and (FINAL) writes its output to slot j = tick - sec
    // -- section 3 writes slot j last, and inputs of slot j were read at the top of this batch or an
    // earlier one.  The last tile of a stream (len < SB_B) steps on the zeros past its end: its end
    // state is not used (the scan reads e_k for k < Tn - 1) and its outputs past len are not stored.
    (void)len;
    T y = 0;
    for (int tau0 = 0; tau0 < SB_B; tau0 += 16) {
        T in[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) in[u] = buf[stl][tau0 + u];
        if (tau0 == 0) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const T left = from_left(y);
                const T xin = sec == 0 ? in[u] : left;
                if (u >= 3 || u >= sec) {
                    y = bq.step(xin);
                    if (FINAL) buf[stl][u - sec] = y;
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const T left = from_left(y);
                y = bq.step(sec == 0 ? in[u] : left);
                if (FINAL) buf[stl][tau0 + u - sec] = y;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) {   // ticks SB_B .. SB_B + 2: sections u+1 .. 3 finish
        const T left = from_left(y);
        if (sec > u) {
            y = bq.step(left);
            if (FINAL) buf[stl][SB_B + u - sec] = y;
        }
    }
    if (!FINAL && own) {
        ends[g * 8 + 2 * sec] = (double)bq.z0;
        ends[g * 8 + 2 * sec + 1] = (double)bq.z1;
    }
    }
    if (!FINAL) return;
    __syncthreads();
    for (int i = tid; i < ST * SB_B; i += SB_LT) {
        const int r = i / SB_B, j = i % SB_B;
        if (r >= nrow) continue;
        const int comp = r & 1, tl = rtile[r], ch = rch[r];
        const long e = (long)tl * SB_B + j;
        if (e >= G.L) continue;
        if (FWD) {
            scr[(size_t)(2 * ch + comp) * G.Lp + e] = buf[r][j];
        } else {   // ext index L-1-e, sample t = ext - pad; decimate keeps t % q == 0
            const long t = G.L - 1 - e - G.pad;
            if (t >= 0 && t < G.N && t % G.q == 0) out[lo.off(ch, t / G.q) + comp] = buf[r][j];
        }
    }
}

// Start states of every tile of one stream (workgroup = stream 2 ch + comp, thread = tile):
// w_0 = sosfilt_zi * ext[0] (T, as the sequential pass computes it), w_k = e_{k-1}; then for
// d = 1, 2, 4, ..: w_k += Phi^d w_{k-d} (k >= d), each product summed in j order without FMA
// (oracle/compat.py: _blocked_scan restates it).
template <typename T, bool FWD>
__global__ __launch_bounds__(1024) void k_sosb_scan(const T *__restrict__ x, const T *__restrict__ scr, SbGeo G,
                                                    const T *__restrict__ zi, const double *__restrict__ phi,
                                                    const double *__restrict__ ends, double *__restrict__ states) {
    __shared__ double w[SB_MAXT][8];
    const int k = threadIdx.x, s = blockIdx.x, ch = s >> 1, comp = s & 1;
    const bool on = k < G.Tn;
    double v[8];
    if (on) {
        if (k == 0) {
            T x0;
            if (FWD) {
                const T *xr = x + (size_t)ch * G.N * 2 + comp;
                x0 = (T)2 * xr[0] - xr[2 * G.pad];
            } else {
                x0 = scr[(size_t)s * G.Lp + G.L - 1];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = (double)(zi[i] * x0);
        } else {
            const double *e = ends + ((size_t)(ch * G.Tn + k - 1) * 2 + comp) * 8;
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = e[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) w[k][i] = v[i];
    }
    for (int r = 0; (1 << r) < G.Tn; ++r) {
        const int d = 1 << r;
        __syncthreads();
        double u[8];
        const bool upd = on && k >= d;
        if (upd) {
#pragma unroll
            for (int i = 0; i < 8; ++i) u[i] = w[k - d][i];
        }
        __syncthreads();
        if (upd) {
            // the table straight from global memory at a wave-uniform address: scalar loads, SGPR
            // operands (staged in LDS, its 36 broadcast reads per level cost ~2 us per scan:
            // profiles/r05_ab_scan_sgpr.txt)
            const double *P = phi + __builtin_amdgcn_readfirstlane(r) * 64;
            // the eight rows' sums side by side (each still j-ascending, no FMA: the same bits), then
            // the new state to LDS
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = v[i] + P[i * 8 + j] * u[j];
#pragma unroll
            for (int i = 0; i < 8; ++i) w[k][i] = v[i];
        }
    }
    if (on) {
        double *o = states + ((size_t)(ch * G.Tn + k) * 2 + comp) * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = v[i];
    }
}
}  // namespace

// A (the cascade's one-sample zero-input transition, from the coefficients the kernels use, in
// double) and the table Phi^(2^r) = A^(SB_B 2^r), r < SB_NPOW, row-major 8 x 8 each; every product
// summed in k order without FMA (the oracle computes the same table the same way).
void blocked_table(const double *coef /*[24] sos rows*/, double *tab /*[SB_NPOW * 64]*/) {
    double A[64];
    for (int k = 0; k < 8; ++k) {
        double z[8] = {0}, zn[8];
        z[k] = 1.0;
        double u = 0.0;
        for (int s = 0; s < NSEC; ++s) {
            const double *c = coef + 6 * s;
            const double xn = c[0] * u + z[2 * s];
            zn[2 * s] = (c[1] * u - c[4] * xn) + z[2 * s + 1];
            zn[2 * s + 1] = c[2] * u - c[5] * xn;
            u = xn;
        }
        for (int i = 0; i < 8; ++i) A[i * 8 + k] = zn[i];
    }
    for (int b = 1; b < SB_B; b <<= 1) mat_square(A, A, 8);   // A^SB_B (SB_B a power of two)
    for (int i = 0; i < 64; ++i) tab[i] = A[i];
    for (int r = 1; r < SB_NPOW; ++r) mat_square(tab + (r - 1) * 64, tab + r * 64, 8);
}

namespace {

// ----------------------------------------------------------------- host-side drivers
// The backward kernel for format T and compiled-in decimation factor QT (0: any q); complex64 runs
// the banked lanes (unique loads, any row length) forward, and backward where QT != 0.
template <typename T, int QT>
const void *sos_bwd_fn() {
    if constexpr (std::is_same<T, float>::value && QT != 0) return reinterpret_cast<const void *>(&k_sos_bwd_bank<QT>);
    else return reinterpret_cast<const void *>(&k_sos_bwd<T, QT>);
}

// Input rows are complex [C][N] (row_major).
template <typename T>
int run_decimate(tetra_ctx *ctx, const tetra_compat_plan *P, const void *xv, int C, long N, void *outv, Lay lo) {
    const T *x = (const T *)xv;
    T *out = (T *)outv;
    int pad = 27, q = P->q;   // 3 * (2*4 + 1): sosfiltfilt default padlen for 4 sections
    const long L = N + 2 * pad;
    long Lp = (L + 3) & ~3L;   // stream-major scratch rows, 16-byte aligned
    T *scr = (T *)ws(ctx, S_W0, (size_t)2 * C * Lp * sizeof(T));
    T *coef = (T *)ws(ctx, S_W7, 32 * sizeof(T));
    if (!scr || !coef) return TETRA_E_NOMEM;
    const int rc = upload_sos_coef(ctx, P, coef);
    if (rc) return rc;
    const T *sos = coef, *zi = coef + 24;
    const void *fwd;
    if constexpr (std::is_same<T, float>::value) fwd = reinterpret_cast<const void *>(&k_sos_fwd_bank);
    else fwd = reinterpret_cast<const void *>(&k_sos_fwd<T, 1>);
    // the decimation factors of 2.4 and 1.8 MSps captures (q = 10, 7) compiled in; others generic
    const void *const bwd[3] = {sos_bwd_fn<T, 10>(), sos_bwd_fn<T, 7>(), sos_bwd_fn<T, 0>()};
    // four waves per workgroup: one per SIMD of a CU.  The 8 C lanes make one wave per SIMD over the
    // chip, and 64-lane workgroups left the placement to the dispatcher
    const unsigned blk = 256;
    const dim3 grid(grid_for((size_t)8 * C, blk));
    {
        PROF(ctx, "compat_sos_fwd");
        void *args[] = {&x, &C, &N, &pad, &sos, &zi, &scr, &Lp};
        (void)hipLaunchKernel(fwd, grid, dim3(blk), args, 0, ctx->stream);
    }
    {
        PROF(ctx, "compat_sos_bwd");
        void *args[] = {&scr, &Lp, &C, &N, &pad, &q, &sos, &zi, &out, &lo};
        (void)hipLaunchKernel(bwd[q == 10 ? 0 : q == 7 ? 1 : 2], grid, dim3(blk), args, 0, ctx->stream);
    }
    return TETRA_OK;
}

// The time-blocked decimator (k_sosb_*): run_decimate's contract, for the shapes of blocked_fits.
template <typename T>
int run_decimate_blocked(tetra_ctx *ctx, const tetra_compat_plan *P, const void *xv, int C, long N, void *outv,
                         Lay lo) {
    const T *x = (const T *)xv;
    T *out = (T *)outv;
    const int pad = 27;
    const long L = N + 2 * pad;
    const long Lp = (L + 3) & ~3L;
    const int Tn = (int)ceil_div(L, SB_B);
    const size_t ntile = (size_t)2 * C * Tn;
    T *scr = (T *)ws(ctx, S_W0, (size_t)2 * C * Lp * sizeof(T));
    T *coef = (T *)ws(ctx, S_W7, 32 * sizeof(T));
    double *sb = (double *)ws(ctx, S_W16, (2 * ntile * 8 + SB_NPOW * 64) * sizeof(double));
    if (!scr || !coef || !sb) return TETRA_E_NOMEM;
    double *ends = sb, *states = sb + ntile * 8, *phi = sb + 2 * ntile * 8;
    double dc[24];
    const int rc = upload_sos_coef(ctx, P, coef, dc);
    if (rc) return rc;
    // the table is a function of the 24 SOS coefficients alone (in the working precision): key the
    // upload on them, not on q, so a caller's own plan with other coefficients never reuses it
    if (!ctx->sosb_valid || ctx->sosb_dev != (const void *)phi || std::memcmp(ctx->sosb_coef, dc, sizeof dc) != 0) {
        ctx->sosb_tab.resize(SB_NPOW * 64);
        blocked_table(dc, ctx->sosb_tab.data());
        HIP_TRY(ctx, hipMemcpyAsync(phi, ctx->sosb_tab.data(), SB_NPOW * 64 * sizeof(double), hipMemcpyHostToDevice,
                                    ctx->stream));
        std::memcpy(ctx->sosb_coef, dc, sizeof dc);
        ctx->sosb_valid = true;
        ctx->sosb_dev = phi;
    }
    const SbGeo G{C, Tn, pad, P->q, N, L, Lp};
    constexpr int ST = SbCfg<T>::ST;
    const dim3 gt((unsigned)ceil_div((long)ntile, ST)), bt(SB_LT);
    const dim3 gs((unsigned)(2 * C)), bs((unsigned)std::min(SB_MAXT, (int)ceil_div(Tn, 64) * 64));
    // a pass: the tiles' end states from zero, the scan to their start states, the outputs to o
    auto pass = [&](const char *stage, auto ends_of, auto scan, auto final, T *o) {
        PROF(ctx, stage);
        hipLaunchKernelGGL(ends_of, gt, bt, 0, ctx->stream, x, scr, G, coef, nullptr, ends, (T *)nullptr, lo);
        hipLaunchKernelGGL(scan, gs, bs, 0, ctx->stream, x, scr, G, coef + 24, phi, ends, states);
        hipLaunchKernelGGL(final, gt, bt, 0, ctx->stream, x, scr, G, coef, states, nullptr, o, lo);
    };
    pass("compat_sosb_fwd", k_sosb_tile<T, true, false>, k_sosb_scan<T, true>, k_sosb_tile<T, true, true>, (T *)nullptr);
    pass("compat_sosb_bwd", k_sosb_tile<T, false, false>, k_sosb_scan<T, false>, k_sosb_tile<T, false, true>, out);
    HIP_TRY(ctx, hipGetLastError());
    return TETRA_OK;
}

}  // namespace

int compat_decimate(tetra_ctx *ctx, const tetra_compat_plan *P, int fmt, DecForm form, const void *x, int C, long N,
                    void *out, Lay lo) {
    if (form == DEC_TILED)
        return run_decimate_tiled(ctx, P, (const float *)x, C, N, (float *)out, lo.s_grp, lo.s_n, lo.s_lane);
    const bool f64 = fmt == TETRA_CF64;
    if (form == DEC_BLOCKED)
        return f64 ? run_decimate_blocked<double>(ctx, P, x, C, N, out, lo)
                   : run_decimate_blocked<float>(ctx, P, x, C, N, out, lo);
    return f64 ? run_decimate<double>(ctx, P, x, C, N, out, lo) : run_decimate<float>(ctx, P, x, C, N, out, lo);
}

extern "C" int tetra_decimate(tetra_ctx *ctx, const tetra_compat_plan *P, const void *iq, int fmt, size_t C, size_t N,
                              void *out) {
    if (!ctx) return TETRA_E_INVALID;
    int rc = check_plan(ctx, P);
    if (rc) return rc;
    if (P->q < 2 || N <= 27 || C == 0) return tetra_fail(ctx, TETRA_E_INVALID, "decimate needs q>=2 and N>27");
    const size_t es = compat_elem_size(ctx, fmt);
    if (!es) return TETRA_E_INVALID;
    const long M = ceil_div((long)N, P->q);
    Staging st(ctx);
    const void *x = st.in(iq, C * N * 2 * es);
    void *o = st.out(out, C * M * 2 * es);
    if (!x || !o) return st.finish();
    rc = compat_decimate(ctx, P, fmt, DEC_SEQUENTIAL, x, (int)C, (long)N, o, row_major(M));
    if (rc) return rc;
    return st.finish();
}
