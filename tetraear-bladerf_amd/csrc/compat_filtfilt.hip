// compat_filtfilt.hip -- stage 2 of the compat chain (compat_demod.hip: numerics, layouts):
// frequency_shift and filter_signal (butter(4) + filtfilt, odd pad 15, complex128), sequential in
// time or, opt-in, time-blocked; and the ETSI receiver's streaming AFC mixer (the same arithmetic).
#include "common.h"
#include "compat_sos.h"   // Lay, the tile geometry, the stage entry points

namespace {

// ------------------------------------------------------------------ mixer + filtfilt (lfilter)
// Value of component `comp` of (possibly frequency-shifted) sample n, in double.
__device__ __forceinline__ double mix_pair(double xr, double xi, long n, int comp, bool mix, double c, double fs) {
    if (!mix) return comp ? xi : xr;
    // numpy: t = arange/fs; arg = (-1j*2*pi*f)*t has real part 0, imag c*t; exp(arg) = (cos, sin)
    const double th = c * ((double)n / fs);
    double s, co;
    sincos(th, &s, &co);
    // numpy SIMD complex multiply: re = fma(xr, sr, -(xi*si)), im = fma(xr, si, xi*sr)
    return comp ? fma(xr, s, xi * co) : fma(xr, co, -(xi * s));
}

template <typename TIn>
__device__ __forceinline__ double mixed_val(const TIn *xp, size_t sx, long n, int comp, bool mix, double c,
                                            double fs) {
    const double xr = (double)xp[(size_t)n * sx], xi = (double)xp[(size_t)n * sx + 1];
    if (!mix) return comp ? xi : xr;
    // numpy: t = arange/fs; arg = (-1j*2*pi*f)*t has real part 0, imag c*t; exp(arg) = (cos, sin)
    const double th = c * ((double)n / fs);
    double s, co;
    sincos(th, &s, &co);
    // numpy SIMD complex multiply: re = fma(xr, sr, -(xi*si)), im = fma(xr, si, xi*sr)
    return comp ? fma(xr, s, xi * co) : fma(xr, co, -(xi * s));
}

// Odd-extended input of filtfilt at ext index j.  The extension is computed in the precision of
// the array filtfilt receives: complex128 when mixed, else the input type (complex64 from
// decimate), then promoted to double (scipy lfilter runs in complex128).
template <typename TIn>
__device__ __forceinline__ double lf_ext(const TIn *xp, size_t sx, long M, int pad, long j, int comp, bool mix,
                                         double c, double fs) {
    long n;
    int side;
    if (j < pad) { n = pad - j; side = -1; }
    else if (j < pad + M) { n = j - pad; side = 0; }
    else { n = M - 2 - (j - pad - M); side = 1; }
    if (mix) {
        const double v = mixed_val(xp, sx, n, comp, true, c, fs);
        if (side == 0) return v;
        const double e = mixed_val(xp, sx, side < 0 ? 0 : M - 1, comp, true, c, fs);
        return 2.0 * e - v;
    }
    const TIn v = xp[(size_t)n * sx + comp];
    if (side == 0) return (double)v;
    const TIn e = xp[(size_t)(side < 0 ? 0 : M - 1) * sx + comp];
    return (double)((TIn)2 * e - v);
}

constexpr int MAXTAP = 8;

// scipy lfilter (DF-II-T) with NT taps, one stream (channel x re|im) per lane, in double:
//   y = z0 + b0*x;  z_k = (z_{k+1} + x*b_{k+1}) - y*a_{k+1};  z_{NT-2} = x*b_{NT-1} - y*a_{NT-1}
template <int NT>
struct Lfilt {
    double bb[NT], aa[NT], z[NT - 1];
    __device__ __forceinline__ void init(const double *b, const double *a, const double *zi, double x0) {
#pragma unroll
        for (int k = 0; k < NT; ++k) { bb[k] = b[k]; aa[k] = a[k]; }
#pragma unroll
        for (int k = 0; k < NT - 1; ++k) z[k] = zi[k] * x0;
    }
    __device__ __forceinline__ double step(double xn) {
        const double yn = z[0] + bb[0] * xn;
#pragma unroll
        for (int k = 0; k < NT - 2; ++k) z[k] = (z[k + 1] + xn * bb[k + 1]) - yn * aa[k + 1];
        z[NT - 2] = xn * bb[NT - 1] - yn * aa[NT - 1];
        return yn;
    }
};

// The same lfilter with its four states spread over a quad of lanes (NT = 5: butter(4)): lane k holds
// z_k; per sample every lane forms y = z_0 + b0 x from quad lane 0's state (DPP broadcast), and
// z_k = (z_{k+1} + x b_{k+1}) - y a_{k+1} from lane k+1's (DPP shift; lane 3: x b_4 - y a_4).  The
// operations and their order are Lfilt's; a sample is 5 float64 operations per wave instead of 17.
template <int CTRL>
__device__ __forceinline__ double dpp64(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    // quad_perm writes every lane: no `old` operand to materialise
    const int lo = __builtin_amdgcn_mov_dpp((int)(b & 0xffffffff), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xf, 0xf, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
struct Lfilt4 {
    double b0, bk, ak, z;
    bool last;
    __device__ __forceinline__ void init(const double *b, const double *a, const double *zi, double x0) {
        const int k = threadIdx.x & 3;
        b0 = b[0];
        bk = b[k + 1];
        ak = a[k + 1];
        z = zi[k] * x0;
        last = k == 3;
    }
    __device__ __forceinline__ double step(double xn) {
        const double z0 = dpp64<0x00>(z);   // quad_perm [0,0,0,0]: lane 0's z_0
        const double zs = dpp64<0xF9>(z);   // quad_perm [1,2,3,3]: lane k+1's z_{k+1}
        const double yn = z0 + b0 * xn;
        const double t = xn * bk;
        z = (last ? t : zs + t) - yn * ak;
        return yn;
    }
};
// Lanes per stream of the filtfilt kernels: 4 (Lfilt4) for a few channels, where one wave's issue
// sets the time -- one 131072-sample chunk (C2): filtfilt 1.97 -> ~1.7 ms, process() 7.2 -> 7.0 ms --
// and 1 (Lfilt) for batches, which are bound by the load path: at 8192 channels Lfilt4's four lanes
// per stream make the two passes 1.04 + 0.75 -> 1.30 + 0.99 ms (profiles/r06_ab_compat_lf4.txt).
// TETRA_COMPAT_LF=1 / 4 forces a form (same-box A/B).
constexpr int LF4_MAXC = 64;
static int lf_lanes(int C) {
    const char *e = getenv("TETRA_COMPAT_LF");
    if (e && (atoi(e) == 1 || atoi(e) == 4)) return atoi(e);
    return C <= LF4_MAXC ? 4 : 1;
}

constexpr int LFB = 16;   // samples per load batch; batches double-buffered

// Forward pass over the odd extension (filtfilt padlen 3*NT) of the (optionally mixed) input.
// MIX = false (launched when no channel mixes, e.g. on k_mix's pre-mixed rows): the mixer's sincos
// code leaves the loop -- with it inlined 16 times the kernel holds values in AGPRs across the
// recursion; the same operations otherwise.
// QL lanes per stream: 1 (Lfilt) or 4 (Lfilt4, NT = 5: the quad's four lanes hold the same y and all
// store it -- one address, one value -- so no per-sample branch).
template <typename TIn, int NT, bool MIX = true, int QL = 1>
__global__ __launch_bounds__(64) void k_lf_fwd(const TIn *__restrict__ x, Lay lx, int C, long M, int pad,
                                               const double *__restrict__ b, const double *__restrict__ a,
                                               const double *__restrict__ zi, const double *__restrict__ mixc,
                                               const uint8_t *__restrict__ mixon, double fs,
                                               double *__restrict__ scr, Lay ls) {
    static_assert(QL == 1 || (QL == 4 && NT == 5), "Lfilt4 holds butter(4)'s four states");
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int ch = (gid / QL) >> 1, comp = (gid / QL) & 1;
    constexpr bool st = true;
    if (ch >= C) return;   // whole quads
    const bool mix = MIX && mixon && mixon[ch];
    const double c = mix ? mixc[ch] : 0.0;
    const TIn *xp = x + lx.off(ch, 0);
    const size_t sx = lx.s_n;
    const long L = M + 2 * pad;
    typename std::conditional<QL == 4, Lfilt4, Lfilt<NT>>::type f;
    f.init(b, a, zi, lf_ext(xp, sx, M, pad, 0, comp, mix, c, fs));
    double *sp = scr + ls.off(ch, 0) + comp;
    const size_t ss = ls.s_n;
    long j = 0;
    for (; j < pad; ++j) {
        const double yv = f.step(lf_ext(xp, sx, M, pad, j, comp, mix, c, fs));
        if (st) sp[(size_t)j * ss] = yv;
    }
    // body: a batch's 16 (re, im) loads issue together, one batch ahead of the recursion; the
    // mixer (a divergent sincos branch) runs between load and recursion
    using P2 = typename std::conditional<sizeof(TIn) == 4, float2, double2>::type;
    const P2 *xq = reinterpret_cast<const P2 *>(xp);   // (re, im) of sample n at xq[n * sx / 2]
    const size_t sq = sx / 2;
    P2 ra[LFB], rb[LFB];
    auto ld = [&](P2 (&r)[LFB], long j0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < LFB; ++u) r[u] = xq[(size_t)(j0 + u - pad) * sq];
    };
    auto run = [&](P2 (&r)[LFB], long j0) __attribute__((always_inline)) {
        double xs[LFB];
#pragma unroll
        for (int u = 0; u < LFB; ++u) xs[u] = mix_pair((double)r[u].x, (double)r[u].y, j0 + u - pad, comp, mix, c, fs);
#pragma unroll
        for (int u = 0; u < LFB; ++u) {
            const double yv = f.step(xs[u]);
            if (st) sp[(size_t)(j0 + u) * ss] = yv;
        }
    };
    if (M >= 2 * LFB) {
        ld(ra, j);
        ld(rb, j + LFB);
        for (; j + 4 * LFB <= pad + M; j += 2 * LFB) {
            run(ra, j);
            __builtin_amdgcn_sched_barrier(0);
            ld(ra, j + 2 * LFB);
            run(rb, j + LFB);
            __builtin_amdgcn_sched_barrier(0);
            ld(rb, j + 3 * LFB);
        }
        run(ra, j);
        run(rb, j + LFB);
        j += 2 * LFB;
    }
    for (; j < L; ++j) {
        const double yv = f.step(lf_ext(xp, sx, M, pad, j, comp, mix, c, fs));
        if (st) sp[(size_t)j * ss] = yv;
    }
}

// Reverse pass: y[t] = output at ext index t + pad, t in [0, M).
template <int NT, int QL = 1>
__global__ __launch_bounds__(64) void k_lf_bwd(const double *__restrict__ scr, Lay ls, int C, long M, int pad,
                                               const double *__restrict__ b, const double *__restrict__ a,
                                               const double *__restrict__ zi, double *__restrict__ out, Lay lo) {
    static_assert(QL == 1 || (QL == 4 && NT == 5), "Lfilt4 holds butter(4)'s four states");
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int ch = (gid / QL) >> 1, comp = (gid / QL) & 1;
    constexpr bool st = true;
    if (ch >= C) return;   // whole quads
    const double *sp = scr + ls.off(ch, 0) + comp;
    const size_t ss = ls.s_n;
    const long L = M + 2 * pad;
    typename std::conditional<QL == 4, Lfilt4, Lfilt<NT>>::type f;
    f.init(b, a, zi, sp[(size_t)(L - 1) * ss]);
    double *op = out + lo.off(ch, 0) + comp;
    const size_t so = lo.s_n;
    long j = L - 1;
    for (; j >= pad + M; --j) f.step(sp[(size_t)j * ss]);   // end padding: no output
    double xa[LFB], xb[LFB];
    auto ld = [&](double (&v)[LFB], long j0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < LFB; ++u) v[u] = sp[(size_t)(j0 - u) * ss];
    };
    auto run = [&](double (&v)[LFB], long j0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < LFB; ++u) {
            const double yv = f.step(v[u]);
            if (st) op[(size_t)(j0 - u - pad) * so] = yv;
        }
    };
    if (j - 2 * LFB + 1 >= pad) {
        ld(xa, j);
        ld(xb, j - LFB);
        for (; j - 4 * LFB + 1 >= pad; j -= 2 * LFB) {
            run(xa, j);
            __builtin_amdgcn_sched_barrier(0);
            ld(xa, j - 2 * LFB);
            run(xb, j - LFB);
            __builtin_amdgcn_sched_barrier(0);
            ld(xb, j - 3 * LFB);
        }
        run(xa, j);
        run(xb, j - LFB);
        j -= 2 * LFB;
    }
    for (; j >= 0; --j) {
        const double yn = f.step(sp[(size_t)j * ss]);
        if (st && j >= pad) op[(size_t)(j - pad) * so] = yn;
    }
}

// ------------------------------------------------------------------ time-blocked filtfilt (latency mode)
// filter_signal's lfilter passes for a few channels, parallel in time like the decimator above: one
// lane per (channel, component, tile of LB_B samples), the tile's input -- the odd extension of the
// (mixed) decimated samples, each mixed in parallel as it is loaded -- staged in LDS; pass 1 from zero
// state gives each tile's end state (the 4 DF-II-T states), k_lfb_scan the true start states in
// float64 (Psi = B^LB_B, B the one-sample zero-input transition of scipy's lfilter loop), pass 2
// the outputs.  Everything is float64, so the outputs differ from scipy's sequential pass by float64
// rounding only (oracle/compat.py: filtfilt_blocked restates it; the GPU equals it bit for bit).
constexpr int LB_ST = 16;        // stream-tiles per workgroup (one lane of wave 0 each): one channel's
                                 // tiles spread over many CUs, 8 staged samples (and mixers) per thread
constexpr int LB_T = 256;        // threads per workgroup: all four waves stage the tiles

struct LbGeo {
    int C, Tn, pad;
    long M, L;
};

// stream-tile g = (ch * Tn + tile) * 2 + comp
template <typename TIn, bool FWD, bool FINAL>
__global__ __launch_bounds__(LB_T) void k_lfb_tile(const TIn *__restrict__ x, Lay lx, const double *__restrict__ mixc,
                                                    const uint8_t *__restrict__ mixon, double fs,
                                                    double *__restrict__ scr, Lay ls, LbGeo G,
                                                    const double *__restrict__ b, const double *__restrict__ a,
                                                    const double *__restrict__ states, double *__restrict__ ends,
                                                    double *__restrict__ out, Lay lo) {
    __shared__ double buf[LB_ST][LB_B + 1];
    __shared__ int rch[LB_ST], rtile[LB_ST];   // the rows' channel and tile (one division per row)
    const int tid = threadIdx.x;
    const long ntiles = (long)2 * G.C * G.Tn;
    const int nrow = (int)min((long)LB_ST, ntiles - (long)blockIdx.x * LB_ST);
    if (tid < LB_ST) {
        const int pr = (int)((((long)blockIdx.x * LB_ST + (tid < nrow ? tid : 0))) >> 1);
        rtile[tid] = pr % G.Tn;
        rch[tid] = pr / G.Tn;
    }
    __syncthreads();
    // cooperative load by all LB_T threads, 8 loads in flight per thread (unconditional, clamped),
    // then each element's value: lf_ext's arithmetic (mixer, odd extension) on the loaded samples
    constexpr int PER = LB_ST * LB_B / LB_T, U = 8;
    using P2 = typename std::conditional<sizeof(TIn) == 4, float2, double2>::type;
    auto where = [&](int i, int &r, int &j, long &e, int &ch, int &comp, bool &in) {
        r = i / LB_B;
        j = i % LB_B;
        in = r < nrow;
        const int rr = in ? r : 0;
        comp = rr & 1;   // LB_ST is even
        const int tile = rtile[rr];
        ch = rch[rr];
        e = (long)tile * LB_B + j;
        in = in && e < G.L;
        if (!in) e = 0;
    };
    for (int c0 = 0; c0 < PER; c0 += U) {
        P2 raw[U];      // forward: the input pair
        double rb[U];   // backward: the scratch value
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int r, j, ch, comp;
            long e;
            bool in;
            where(tid + LB_T * (c0 + u), r, j, e, ch, comp, in);
            if (FWD) {   // the (re, im) pair of the sample lf_ext reflects (or copies) at ext index e
                const long n = e < G.pad ? G.pad - e : (e < G.pad + G.M ? e - G.pad : G.M - 2 - (e - G.pad - G.M));
                raw[u] = *reinterpret_cast<const P2 *>(x + lx.off(ch, 0) + (size_t)n * lx.s_n);
            } else {
                rb[u] = scr[ls.off(ch, G.L - 1 - e) + comp];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int r, j, ch, comp;
            long e;
            bool in;
            where(tid + LB_T * (c0 + u), r, j, e, ch, comp, in);
            double v = 0.0;
            if (in) {
                if (FWD) {
                    const bool mix = mixon && mixon[ch];
                    const int side = e < G.pad ? -1 : (e < G.pad + G.M ? 0 : 1);
                    const long n = side < 0 ? G.pad - e : (side == 0 ? e - G.pad : G.M - 2 - (e - G.pad - G.M));
                    if (mix) {   // mixed_val on the loaded pair, then the extension in double
                        const double c = mixc[ch];
                        const double th = c * ((double)n / fs);
                        double sn, co;
                        sincos(th, &sn, &co);
                        const double xr = (double)raw[u].x, xi = (double)raw[u].y;
                        v = comp ? fma(xr, sn, xi * co) : fma(xr, co, -(xi * sn));
                        if (side != 0)
                            v = 2.0 * mixed_val(x + lx.off(ch, 0), lx.s_n, side < 0 ? 0 : G.M - 1, comp, true, c, fs) - v;
                    } else {     // the extension in the input precision, then promoted
                        const TIn vv = comp ? raw[u].y : raw[u].x;
                        if (side == 0) {
                            v = (double)vv;
                        } else {
                            const TIn ev = x[lx.off(ch, side < 0 ? 0 : G.M - 1) + comp];
                            v = (double)((TIn)2 * ev - vv);
                        }
                    }
                } else {
                    v = rb[u];
                }
            }
            buf[r][j] = v;
        }
    }
    __syncthreads();
    // the recursion: one lane of wave 0 per stream-tile
    const int row = tid < LB_ST ? tid : 0;
    const long g = (long)blockIdx.x * LB_ST + row;
    const bool own = tid < LB_ST && g < ntiles;
    const int tile = own ? (int)((g >> 1) % G.Tn) : 0;
    const int len = own ? (int)min((long)LB_B, G.L - (long)tile * LB_B) : 0;
    Lfilt<LB_NS + 1> f;
#pragma unroll
    for (int k = 0; k <= LB_NS; ++k) { f.bb[k] = b[k]; f.aa[k] = a[k]; }
#pragma unroll
    for (int k = 0; k < LB_NS; ++k) f.z[k] = (FINAL && own) ? states[g * LB_NS + k] : 0.0;
    // every tile runs all LB_B steps: the last tile of a stream (len < LB_B) steps on the zeros past
    // its end -- its end state is not used by the scan and its outputs past len are not stored
    (void)len;
    for (int j0 = 0; j0 < (tid < LB_ST ? LB_B : 0); j0 += 16) {   // wave 0 only (wave-uniform)
        double in[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) in[u] = buf[row][j0 + u];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const double y = f.step(in[u]);
            if (FINAL) buf[row][j0 + u] = y;
        }
    }
    if (!FINAL) {
        if (own) {
#pragma unroll
            for (int k = 0; k < LB_NS; ++k) ends[g * LB_NS + k] = f.z[k];
        }
        return;
    }
    __syncthreads();
    for (int i = tid; i < LB_ST * LB_B; i += LB_T) {
        const int r = i / LB_B, j = i % LB_B;
        if (r >= nrow) continue;
        const int comp = r & 1, tl = rtile[r], ch = rch[r];
        const long e = (long)tl * LB_B + j;
        if (e >= G.L) continue;
        if (FWD) {
            scr[ls.off(ch, e) + comp] = buf[r][j];
        } else {   // ext index L-1-e -> output t = ext - pad
            const long t = G.L - 1 - e - G.pad;
            if (t >= 0 && t < G.M) out[lo.off(ch, t) + comp] = buf[r][j];
        }
    }
}

// Start states of every tile of one stream (workgroup = stream 2 ch + comp, thread = tile), as
// k_sosb_scan: w_0 = zi * ext[0] (forward) or zi * scr[L-1] (backward), w_k = e_{k-1};
// w_k += Psi^d w_{k-d} for d = 1, 2, 4, .., products summed in j order without FMA.
template <typename TIn, bool FWD>
__global__ __launch_bounds__(1024) void k_lfb_scan(const TIn *__restrict__ x, Lay lx, const double *__restrict__ mixc,
                                                   const uint8_t *__restrict__ mixon, double fs,
                                                   const double *__restrict__ scr, Lay ls, LbGeo G,
                                                   const double *__restrict__ zi, const double *__restrict__ psi,
                                                   const double *__restrict__ ends, double *__restrict__ states) {
    __shared__ double w[SB_MAXT][LB_NS];
    const int k = threadIdx.x, s = blockIdx.x, ch = s >> 1, comp = s & 1;
    const bool on = k < G.Tn;
    double v[LB_NS];
    if (on) {
        if (k == 0) {
            double x0;
            if (FWD) {
                const bool mix = mixon && mixon[ch];
                x0 = lf_ext(x + lx.off(ch, 0), lx.s_n, G.M, G.pad, 0, comp, mix, mix ? mixc[ch] : 0.0, fs);
            } else {
                x0 = scr[ls.off(ch, G.L - 1) + comp];
            }
#pragma unroll
            for (int i = 0; i < LB_NS; ++i) v[i] = zi[i] * x0;
        } else {
            const double *e = ends + ((size_t)(ch * G.Tn + k - 1) * 2 + comp) * LB_NS;
#pragma unroll
            for (int i = 0; i < LB_NS; ++i) v[i] = e[i];
        }
#pragma unroll
        for (int i = 0; i < LB_NS; ++i) w[k][i] = v[i];
    }
    for (int r = 0; (1 << r) < G.Tn; ++r) {
        const int d = 1 << r;
        __syncthreads();
        double u[LB_NS];
        const bool upd = on && k >= d;
        if (upd) {
#pragma unroll
            for (int i = 0; i < LB_NS; ++i) u[i] = w[k - d][i];
        }
        __syncthreads();
        if (upd) {
            const double *P = psi + (size_t)r * LB_NS * LB_NS;
#pragma unroll
            for (int i = 0; i < LB_NS; ++i) {
                double acc = v[i];
#pragma unroll
                for (int j = 0; j < LB_NS; ++j) acc = acc + P[i * LB_NS + j] * u[j];
                v[i] = acc;
                w[k][i] = acc;
            }
        }
    }
    if (on) {
        double *o = states + ((size_t)(ch * G.Tn + k) * 2 + comp) * LB_NS;
#pragma unroll
        for (int i = 0; i < LB_NS; ++i) o[i] = v[i];
    }
}
}  // namespace

// B (scipy lfilter's one-sample zero-input transition of the 4 DF-II-T states) and the table
// Psi^(2^r) = B^(LB_B 2^r), r < SB_NPOW, row-major 4 x 4 each; products summed in k order, no FMA.
void lfilter_table(const double *bcoef, const double *acoef, double *tab /*[SB_NPOW * 16]*/) {
    constexpr int K = LB_NS;
    double Bm[K * K];
    for (int c = 0; c < K; ++c) {
        double z[K] = {0}, zn[K];
        z[c] = 1.0;
        const double xn = 0.0;
        const double yn = z[0] + bcoef[0] * xn;
        for (int k = 0; k < K - 1; ++k) zn[k] = (z[k + 1] + xn * bcoef[k + 1]) - yn * acoef[k + 1];
        zn[K - 1] = xn * bcoef[K] - yn * acoef[K];
        for (int i = 0; i < K; ++i) Bm[i * K + c] = zn[i];
    }
    for (int n = 1; n < LB_B; n <<= 1) mat_square(Bm, Bm, K);
    for (int i = 0; i < K * K; ++i) tab[i] = Bm[i];
    for (int r = 1; r < SB_NPOW; ++r) mat_square(tab + (r - 1) * K * K, tab + r * K * K, K);
}

namespace {

// frequency_shift alone (component API, and the unfiltered-but-shifted process() path).
template <typename TIn>
__global__ __launch_bounds__(256) void k_mix(const TIn *__restrict__ x, Lay lx, int C, long N,
                                             const double *__restrict__ mixc, const uint8_t *__restrict__ mixon,
                                             double fs, double *__restrict__ out, Lay lo) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int ch = (int)(gid / N);
    const long n = gid - (long)ch * N;
    if (ch >= C) return;
    const bool mix = !mixon || mixon[ch];
    const TIn *xp = x + lx.off(ch, 0);
    double *op = out + lo.off(ch, n);
    op[0] = mixed_val(xp, lx.s_n, n, 0, mix, mixc[ch], fs);
    op[1] = mixed_val(xp, lx.s_n, n, 1, mix, mixc[ch], fs);
}

// The ETSI receiver's AFC mixer on a streaming window (tetra_etsi_mix): frequency_shift's
// arithmetic (mixed_val: theta = c (n / fs) in float64, sincos, numpy's complex product) with n the
// GLOBAL sample index n0 + i of the capture, rounded to cf32 -- so consecutive windows of one capture
// are mixed with one continuous phase, and the first (n0 = 0) equals the chunk mixed from its start.
__global__ __launch_bounds__(256) void k_mix_at(const float *__restrict__ x, long ld, int C, long N,
                                                const double *__restrict__ mixc, double fs, long n0,
                                                float *__restrict__ out) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int ch = (int)(gid / N);
    const long i = gid - (long)ch * N;
    if (ch >= C) return;
    const float *xp = x + 2 * ((size_t)ch * ld + i);
    const double xr = (double)xp[0], xi = (double)xp[1];
    const double th = mixc[ch] * ((double)(n0 + i) / fs);
    double sn, co;
    sincos(th, &sn, &co);
    out[2 * ((size_t)ch * N + i)] = (float)fma(xr, co, -(xi * sn));
    out[2 * ((size_t)ch * N + i) + 1] = (float)fma(xr, sn, xi * co);
}

// ----------------------------------------------------------------- host-side drivers
// b, a and lfilter_zi at a pitch of MAXTAP words (the blocked driver puts its Psi table behind them)
void lf_coef_image(const tetra_compat_plan *P, double *hc /*[3 * MAXTAP], zeroed*/) {
    for (int k = 0; k < P->ntaps; ++k) { hc[k] = P->b[k]; hc[MAXTAP + k] = P->a[k]; }
    for (int k = 0; k < P->ntaps - 1; ++k) hc[2 * MAXTAP + k] = P->lzi[k];
}

template <typename TIn>
int run_filtfilt(tetra_ctx *ctx, const tetra_compat_plan *P, const void *xv, Lay lx, int C, long M,
                 const double *mixc, const uint8_t *mixon, double *out, Lay lo) {
    const TIn *x = (const TIn *)xv;
    const int nt = P->ntaps, pad = 3 * nt;
    if (nt != 5) return tetra_fail(ctx, TETRA_E_INVALID, "ntaps %d unsupported (butter(4) has 5)", nt);
    const long L = M + 2 * pad;
    double *scr = (double *)ws(ctx, S_W2, grouped_elems(C, L) * sizeof(double));
    double *coef = (double *)ws(ctx, S_W6, 3 * MAXTAP * sizeof(double));
    if (!scr || !coef) return TETRA_E_NOMEM;
    double hc[3 * MAXTAP] = {0};
    lf_coef_image(P, hc);
    HIP_TRY(ctx, hipMemcpyAsync(coef, hc, sizeof hc, hipMemcpyHostToDevice, ctx->stream));
    const unsigned blk = 64;
    const int ql = lf_lanes(C);
    {
        PROF(ctx, "compat_filtfilt_fwd");
        const dim3 g1(grid_for((size_t)2 * C, blk)), g4(grid_for((size_t)8 * C, blk));
        const Lay ls = grouped(L);
        const double *cb = coef, *ca = coef + MAXTAP, *cz = coef + 2 * MAXTAP;
        // the mixer compiled out when no row mixes
        auto fwd = ql == 4 ? (mixon ? k_lf_fwd<TIn, 5, true, 4> : k_lf_fwd<TIn, 5, false, 4>)
                           : (mixon ? k_lf_fwd<TIn, 5, true, 1> : k_lf_fwd<TIn, 5, false, 1>);
        hipLaunchKernelGGL(fwd, ql == 4 ? g4 : g1, dim3(blk), 0, ctx->stream, x, lx, C, M, pad, cb, ca, cz, mixc, mixon,
                           P->fs_dec, scr, ls);
    }
    {
        PROF(ctx, "compat_filtfilt_bwd");
        hipLaunchKernelGGL((ql == 4 ? k_lf_bwd<5, 4> : k_lf_bwd<5, 1>), dim3(grid_for((size_t)2 * ql * C, blk)), dim3(blk),
                           0, ctx->stream, scr, grouped(L), C, M, pad, coef, coef + MAXTAP, coef + 2 * MAXTAP, out, lo);
    }
    return TETRA_OK;
}

template <typename TIn>
int run_filtfilt_blocked(tetra_ctx *ctx, const tetra_compat_plan *P, const void *xv, Lay lx, int C, long M,
                         const double *mixc, const uint8_t *mixon, double *out, Lay lo) {
    const TIn *x = (const TIn *)xv;
    const int nt = P->ntaps, pad = 3 * nt;
    const long L = M + 2 * pad;
    const int Tn = (int)ceil_div(L, LB_B);
    const size_t ntile = (size_t)2 * C * Tn;
    double *scr = (double *)ws(ctx, S_W2, grouped_elems(C, L) * sizeof(double));
    double *coef = (double *)ws(ctx, S_W6, (3 * MAXTAP + SB_NPOW * LB_NS * LB_NS) * sizeof(double));
    double *lb = (double *)ws(ctx, S_W17, 2 * ntile * LB_NS * sizeof(double));
    if (!scr || !coef || !lb) return TETRA_E_NOMEM;
    double hc[3 * MAXTAP + SB_NPOW * LB_NS * LB_NS] = {0};
    lf_coef_image(P, hc);
    lfilter_table(P->b, P->a, hc + 3 * MAXTAP);
    HIP_TRY(ctx, hipMemcpyAsync(coef, hc, sizeof hc, hipMemcpyHostToDevice, ctx->stream));
    double *ends = lb, *states = lb + ntile * LB_NS;
    const double *psi = coef + 3 * MAXTAP;
    const LbGeo G{C, Tn, pad, M, L};
    const dim3 gt((unsigned)ceil_div((long)ntile, LB_ST)), bt(LB_T);
    const dim3 gs((unsigned)(2 * C)), bs((unsigned)std::min(SB_MAXT, (int)ceil_div(Tn, 64) * 64));
    const Lay ls = grouped(L);
    // a pass: the tiles' end states from zero, the scan to their start states, the outputs to o
    auto pass = [&](const char *stage, auto ends_of, auto scan, auto final, double *o) {
        PROF(ctx, stage);
        hipLaunchKernelGGL(ends_of, gt, bt, 0, ctx->stream, x, lx, mixc, mixon, P->fs_dec, scr, ls, G, coef,
                           coef + MAXTAP, nullptr, ends, nullptr, lo);
        hipLaunchKernelGGL(scan, gs, bs, 0, ctx->stream, x, lx, mixc, mixon, P->fs_dec, scr, ls, G, coef + 2 * MAXTAP,
                           psi, ends, states);
        hipLaunchKernelGGL(final, gt, bt, 0, ctx->stream, x, lx, mixc, mixon, P->fs_dec, scr, ls, G, coef,
                           coef + MAXTAP, states, nullptr, o, lo);
    };
    pass("compat_lfb_fwd", k_lfb_tile<TIn, true, false>, k_lfb_scan<TIn, true>, k_lfb_tile<TIn, true, true>, nullptr);
    pass("compat_lfb_bwd", k_lfb_tile<TIn, false, false>, k_lfb_scan<TIn, false>, k_lfb_tile<TIn, false, true>, out);
    HIP_TRY(ctx, hipGetLastError());
    return TETRA_OK;
}

}  // namespace

int launch_mix(tetra_ctx *ctx, int fmt, const void *x, Lay lx, int C, long N, const double *mixc,
                const uint8_t *mixon, double fs, double *out, Lay lo) {
    const dim3 grid(grid_for((size_t)C * N, 256)), blk(256);
    if (fmt == TETRA_CF64)
        hipLaunchKernelGGL(k_mix<double>, grid, blk, 0, ctx->stream, (const double *)x, lx, C, N, mixc, mixon, fs, out, lo);
    else
        hipLaunchKernelGGL(k_mix<float>, grid, blk, 0, ctx->stream, (const float *)x, lx, C, N, mixc, mixon, fs, out, lo);
    return TETRA_OK;
}

int compat_filtfilt(tetra_ctx *ctx, const tetra_compat_plan *P, int fmt, LfForm form, const void *x, Lay lx, int C,
                    long M, const double *mixc, const uint8_t *mixon, double *out, Lay lo) {
    const bool f64 = fmt == TETRA_CF64;
    if (form == LF_BLOCKED)
        return f64 ? run_filtfilt_blocked<double>(ctx, P, x, lx, C, M, mixc, mixon, out, lo)
                   : run_filtfilt_blocked<float>(ctx, P, x, lx, C, M, mixc, mixon, out, lo);
    if (form == LF_PREMIX) {
        // frequency_shift's values for the whole chunk in parallel first (k_mix: the same mixed_val
        // arithmetic, float64), then the sequential filtfilt on them: bit-identical
        double *pm = (double *)ws(ctx, S_W19, grouped_elems(C, M) * 8);
        if (!pm) return TETRA_E_NOMEM;
        {
            PROF(ctx, "compat_mix");
            (void)launch_mix(ctx, fmt, x, lx, C, M, mixc, mixon, P->fs_dec, pm, grouped(M));
        }
        return run_filtfilt<double>(ctx, P, pm, grouped(M), C, M, nullptr, nullptr, out, lo);
    }
    return f64 ? run_filtfilt<double>(ctx, P, x, lx, C, M, mixc, mixon, out, lo)
               : run_filtfilt<float>(ctx, P, x, lx, C, M, mixc, mixon, out, lo);
}

extern "C" {

int tetra_frequency_shift(tetra_ctx *ctx, const void *iq, int fmt, size_t C, size_t N, const double *mix_c, double fs,
                          void *out) {
    if (!ctx || C == 0) return TETRA_E_INVALID;
    if (N == 0) return TETRA_OK;
    const size_t es = compat_elem_size(ctx, fmt);
    if (!es) return TETRA_E_INVALID;
    Staging st(ctx);
    const void *x = st.in(iq, C * N * 2 * es);
    const double *mc = (const double *)st.in(mix_c, C * sizeof(double));
    void *o = st.out(out, C * N * 16);
    if (!x || !mc || !o) return st.finish();
    (void)launch_mix(ctx, fmt, x, row_major(N), (int)C, (long)N, mc, nullptr, fs, (double *)o, row_major(N));
    return st.finish();
}

int tetra_etsi_mix(tetra_ctx *ctx, const void *iq, size_t C, size_t ld, size_t N, const double *mix_c, double fs,
                   int64_t n0, void *out) {
    if (!ctx || C == 0 || ld < N) return TETRA_E_INVALID;
    if (N == 0) return TETRA_OK;
    Staging st(ctx);
    const float *x = (const float *)st.in(iq, ((C - 1) * ld + N) * 8);
    const double *mc = (const double *)st.in(mix_c, C * sizeof(double));
    float *o = (float *)st.out(out, C * N * 8);
    if (!x || !mc || !o) return st.finish();
    hipLaunchKernelGGL(k_mix_at, dim3(grid_for(C * N, 256)), dim3(256), 0, ctx->stream, x, (long)ld, (int)C, (long)N,
                       mc, fs, (long)n0, o);
    return st.finish();
}

int tetra_filtfilt(tetra_ctx *ctx, const tetra_compat_plan *P, const void *iq, int fmt, size_t C, size_t N, void *out) {
    if (!ctx) return TETRA_E_INVALID;
    if (!P || (long)N <= 3 * P->ntaps || C == 0)
        return tetra_fail(ctx, TETRA_E_INVALID, "filtfilt needs N > padlen");
    const size_t es = compat_elem_size(ctx, fmt);
    if (!es) return TETRA_E_INVALID;
    Staging st(ctx);
    const void *x = st.in(iq, C * N * 2 * es);
    void *o = st.out(out, C * N * 16);
    if (!x || !o) return st.finish();
    const int rc = compat_filtfilt(ctx, P, fmt, LF_SEQUENTIAL, x, row_major(N), (int)C, (long)N, nullptr, nullptr,
                                   (double *)o, row_major(N));
    if (rc) return rc;
    return st.finish();
}

}  // extern "C"
