// compat_symbols.hip -- stages 3 and 4 of the compat chain (compat_demod.hip: numerics, layouts):
// extract_symbols (best integer phase by mean |x|^2, then gather) and demodulate_dqpsk.
#include "common.h"
#include "compat_sos.h"   // Lay, SB_MAXC, the stage entry points

namespace {

// ------------------------------------------------------------------ extract_symbols
// numpy complex |z| (SIMD kernel): larger*sqrt(fma(r, r, 1)), r = smaller/larger.
template <typename T>
__device__ __forceinline__ T np_cabs(T xr, T xi) {
    T re = fabs(xr), im = fabs(xi);
    const T inf = (T)INFINITY;
    const bool re_inf = re == inf, im_inf = im == inf;
    im = re_inf ? inf : im;
    re = im_inf ? inf : re;
    const bool re_ok = !isnan(re), im_ok = !isnan(im);
    im = re_ok ? im : (T)NAN;
    re = im_ok ? re : (T)NAN;
    const T larger = fmax(re, im), smaller = fmin(im, re);
    const bool div_ok = !(larger == (T)0 || smaller == inf);
    const T r = div_ok ? smaller / larger : (T)0;
    return sqrt(fma(r, r, (T)1)) * larger;
}

// extract_symbols' element values |y[n]|^2 (numpy's |z|, squared) for every sample of every channel,
// in parallel: the latency mode's prepass, so k_extract's per-phase pairwise sums read them instead of
// each lane computing its phase's ~1000 |z| one after another.  pw rows [C][M].
template <typename T>
__global__ __launch_bounds__(256) void k_cabs2(const T *__restrict__ y, Lay ly, int C, long M, T *__restrict__ pw) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int ch = (int)(gid / M);
    const long n = gid - (long)ch * M;
    if (ch >= C) return;
    const size_t o = ly.off(ch, n);
    const T a = np_cabs(y[o], y[o + 1]);
    pw[(size_t)ch * M + n] = a * a;
}

// np.mean of v(0..n-1): numpy's pairwise summation (leaf blocks <= 128 with 8 accumulators,
// split point n/2 rounded down to a multiple of 8), then / n.
template <typename T, typename F>
__device__ T pairwise_mean(F v, long n) {
    long st_s[24], st_n[24];
    int st_stage[24];
    T st_left[24];
    int sp = 0;
    st_s[0] = 0; st_n[0] = n; st_stage[0] = 0; sp = 1;
    T ret = 0;
    while (sp > 0) {
        const int top = sp - 1;
        const long s = st_s[top], m = st_n[top];
        if (m <= 128) {
            if (m < 8) {
                T r = 0;
                for (long i = 0; i < m; ++i) r += v(s + i);
                ret = r;
            } else {
                T r[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) r[k] = v(s + k);
                long i = 8;
                for (; i < m - (m % 8); i += 8) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) r[k] += v(s + i + k);
                }
                T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                for (; i < m; ++i) res += v(s + i);
                ret = res;
            }
            --sp;
            continue;
        }
        long n2 = m / 2;
        n2 -= n2 % 8;
        if (st_stage[top] == 0) {
            st_stage[top] = 1;
            st_s[sp] = s; st_n[sp] = n2; st_stage[sp] = 0; ++sp;
        } else if (st_stage[top] == 1) {
            st_left[top] = ret;
            st_stage[top] = 2;
            st_s[sp] = s + n2; st_n[sp] = m - n2; st_stage[sp] = 0; ++sp;
        } else {
            ret = st_left[top] + ret;
            --sp;
        }
    }
    return ret / (T)n;
}

// The same sum as pairwise_mean's, with the tree unrolled at compile time (no stack in scratch, and
// the leaves' loads 16 deep): at most D splits, then leaves of <= 128.  A part after d splits is at
// most n / 2^d + 14 long (each split rounds down to a multiple of 8), so with D = 5 every leaf is
// <= 128 for n <= 3584; callers take pairwise_mean beyond that.  Element i is |y[ph + i sps]|^2; the
// leaf is one out-of-line function (32 inlined copies of its unrolled |z| code would be ~1 MB).
template <typename T>
struct PhasePower {
    const T *yp;
    size_t sy;
    long ph;
    int sps;
    const T *pw;   // the channel's k_cabs2 row, or null: compute |z|^2 here
    __device__ __forceinline__ T operator()(long i) const {
        if (pw) return pw[ph + i * sps];
        const size_t o = (size_t)(ph + i * sps) * sy;
        const T a = np_cabs(yp[o], yp[o + 1]);
        return a * a;
    }
};
template <typename T>
__device__ __noinline__ T pw_leaf(PhasePower<T> v, long s, long m) {
    if (m < 8) {
        T r = 0;
        for (long i = 0; i < m; ++i) r += v(s + i);
        return r;
    }
    T r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = v(s + k);
    long i = 8;
    const long mm = m - (m % 8);
    for (; i + 8 < mm; i += 16) {   // two groups of 8 loads in flight, summed in order
        T a[8], b[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            a[k] = v(s + i + k);
            b[k] = v(s + i + 8 + k);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += a[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += b[k];
    }
    for (; i < mm; i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += v(s + i + k);
    }
    T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < m; ++i) res += v(s + i);
    return res;
}
template <int D, typename T>
__device__ __forceinline__ T pw_sum(const PhasePower<T> &v, long s, long n) {
    if constexpr (D == 0) {
        return pw_leaf<T>(v, s, n);   // n <= 128 here whenever the root's n <= 3584 (see above)
    } else {
        if (n <= 128) return pw_leaf<T>(v, s, n);
        long n2 = n / 2;
        n2 -= n2 % 8;
        const T l = pw_sum<D - 1, T>(v, s, n2);
        const T r = pw_sum<D - 1, T>(v, s + n2, n - n2);
        return l + r;
    }
}

// 16 lanes per channel: lane k tries phase k*step (processor.py:196-210), then the group gathers
// the chosen phase into sym[ch][0..ns).
template <typename T>
__global__ __launch_bounds__(256) void k_extract(const T *__restrict__ y, Lay ly, int C, long M, int sps, int step,
                                                 T *__restrict__ sym, long smax, int32_t *__restrict__ nsym,
                                                 int32_t *__restrict__ bestph, const T *__restrict__ pw = nullptr) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int ch = gid >> 4, k = gid & 15;
    const int lane = threadIdx.x & 63;
    const bool ok = ch < C;
    const int nph = (sps + step - 1) / step;
    const int ph = k * step;
    const T *yp = y + ly.off(ok ? ch : 0, 0);
    const size_t sy = ly.s_n;
    T power = (T)-2;
    long ns = (ok && k < nph) ? (M - ph) / sps : 0;
    if (ns > 0) {
        const PhasePower<T> v{yp, sy, (long)ph, sps, pw ? pw + (size_t)ch * M : nullptr};
        power = ns <= 3584 ? pw_sum<5, T>(v, 0, ns) / (T)ns : pairwise_mean<T>(v, ns);
    }
    T best = (T)-1;
    int bph = 0;
    for (int q = 0; q < nph && q < 16; ++q) {
        const T p = __shfl(power, (lane & ~15) + q, 64);
        const long nq = (M - q * step) / sps;
        if (nq > 0 && p > best) { best = p; bph = q * step; }
    }
    if (!ok) return;
    const long nout = (M - bph) / sps;
    if (k == 0) {
        nsym[ch] = (int32_t)nout;
        if (bestph) bestph[ch] = bph;
    }
    T *op = sym + (size_t)ch * smax * 2;
    for (long i = k; i < nout; i += 16) {
        const size_t o = (size_t)(bph + i * sps) * sy;
        op[2 * i] = yp[o];
        op[2 * i + 1] = yp[o + 1];
    }
}

// Latency mode (a few channels): one 512-thread workgroup per channel, thread = (phase q < 16, leaf
// l < 32).  numpy's pairwise sum of a phase's |y|^2 (pw_sum<5>: splits at n/2 rounded down to a
// multiple of 8 until a part is <= 128, leaves of 8 accumulators) is the same tree here, with its
// <= 32 leaves summed by 32 threads at once and combined in the tree's order by one thread: the same
// adds, so the same power, the same phase and the same symbols as k_extract.  ns <= 3584 per phase
// (five splits); longer chunks take k_extract.
constexpr int XL_LEAVES = 32;
__device__ __forceinline__ int leaf_at(long n, int want, long &s, long &m) {   // DFS leaf `want` of the tree on [0, n)
    long st_s[6], st_n[6];
    int sp = 0, idx = 0;
    st_s[0] = 0;
    st_n[0] = n;
    sp = 1;
    while (sp > 0) {
        --sp;
        const long ss = st_s[sp], nn = st_n[sp];
        if (nn <= 128) {
            if (idx == want) {
                s = ss;
                m = nn;
                return 1;
            }
            ++idx;
            continue;
        }
        long n2 = nn / 2;
        n2 -= n2 % 8;
        st_s[sp] = ss + n2;   // right pushed first: the left child is visited first
        st_n[sp] = nn - n2;
        ++sp;
        st_s[sp] = ss;
        st_n[sp] = n2;
        ++sp;
    }
    return 0;
}
template <int D, typename T>
__device__ T leaf_combine(const T *leaf, int &idx, long n) {   // pw_sum<D>'s adds over the leaf sums
    if constexpr (D == 0) {
        return leaf[idx++];
    } else {
        if (n <= 128) return leaf[idx++];
        long n2 = n / 2;
        n2 -= n2 % 8;
        const T l = leaf_combine<D - 1, T>(leaf, idx, n2);
        const T r = leaf_combine<D - 1, T>(leaf, idx, n - n2);
        return l + r;
    }
}

template <typename T>
__global__ __launch_bounds__(512) void k_extract_lat(const T *__restrict__ y, Lay ly, int C, long M, int sps, int step,
                                                     T *__restrict__ sym, long smax, int32_t *__restrict__ nsym,
                                                     int32_t *__restrict__ bestph, const T *__restrict__ pw) {
    __shared__ T leafs[16][XL_LEAVES];
    __shared__ T power[16];
    __shared__ int bsel;
    const int ch = blockIdx.x, t = threadIdx.x, q = t >> 5, l = t & 31;
    const int nph = (sps + step - 1) / step;
    const int ph = q * step;
    const long ns = q < nph ? (M - ph) / sps : 0;
    const T *yp = y + ly.off(ch, 0);
    if (ns > 0) {
        long s0, m0;
        if (leaf_at(ns, l, s0, m0)) {
            const PhasePower<T> v{yp, ly.s_n, (long)ph, sps, pw + (size_t)ch * M};
            leafs[q][l] = pw_leaf<T>(v, s0, m0);
        }
    }
    __syncthreads();
    if (l == 0) {
        T p = (T)-2;
        if (ns > 0) {
            int idx = 0;
            p = leaf_combine<5, T>(leafs[q], idx, ns) / (T)ns;
        }
        if (q < 16) power[q] = p;
    }
    __syncthreads();
    if (t == 0) {   // k_extract's choice: the first phase of the largest power
        T best = (T)-1;
        int bph = 0;
        for (int qq = 0; qq < nph && qq < 16; ++qq) {
            const long nq = (M - qq * step) / sps;
            if (nq > 0 && power[qq] > best) {
                best = power[qq];
                bph = qq * step;
            }
        }
        bsel = bph;
        nsym[ch] = (int32_t)((M - bph) / sps);
        if (bestph) bestph[ch] = bph;
    }
    __syncthreads();
    const int bph = bsel;
    const long nout = (M - bph) / sps;
    T *op = sym + (size_t)ch * smax * 2;
    for (long i = t; i < nout; i += 512) {
        const size_t o = (size_t)(bph + i * sps) * ly.s_n;
        op[2 * i] = yp[o];
        op[2 * i + 1] = yp[o + 1];
    }
}

// ------------------------------------------------------------------ demodulate_dqpsk
// sym rows [C][stride] complex T, S = nsym[ch] (or S_all); REAL: rows of real T (the reference
// called on a real array: numpy's real division and product, np.imag(diff) = +0).
// BS threads per channel: 64 for batches (one wave per channel), 1024 in the latency mode (a few
// channels: ~1 symbol per thread).  The max is order-independent, so the result is the same.
template <typename T, int BS, bool REAL = false>
__global__ __launch_bounds__(BS) void k_demod(const T *__restrict__ sym, long stride, int C, const int32_t *__restrict__ nsym,
                                              long S_all, double t0, double t1, double t2, double t3,
                                              uint8_t *__restrict__ hard, long hstride) {
    const int ch = blockIdx.x;
    const int lane = threadIdx.x;
    if (ch >= C) return;
    const long S = nsym ? nsym[ch] : S_all;
    if (S < 2) return;
    const T *sp = sym + (size_t)ch * stride * (REAL ? 1 : 2);
    T m = (T)-INFINITY;
    bool any_nan = false;
    for (long k = lane; k < S; k += BS) {
        const T a = REAL ? fabs(sp[k]) : np_cabs(sp[2 * k], sp[2 * k + 1]);
        any_nan |= isnan(a);
        m = fmax(m, a);
    }
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    any_nan = __any(any_nan);
    if constexpr (BS > 64) {   // across the waves
        __shared__ T wm[BS / 64];
        __shared__ int wn[BS / 64];
        if ((lane & 63) == 0) {
            wm[lane >> 6] = m;
            wn[lane >> 6] = any_nan;
        }
        __syncthreads();
        m = wm[0];
        any_nan = wn[0];
        for (int w = 1; w < BS / 64; ++w) {
            m = fmax(m, wm[w]);
            any_nan |= wn[w] != 0;
        }
    }
    const T mx = any_nan ? (T)NAN : m;   // np.max propagates NaN
    // samples / max_power: numpy complex division (Smith) by (m + 0j): rat = 0/m, scl = 1/m,
    // out = ((xr + xi*rat)*scl, (xi - xr*rat)*scl)
    const bool norm = mx > (T)0;
    const T rat = norm ? (T)0 / mx : (T)0;
    const T scl = norm ? (T)1 / (mx + (T)0 * rat) : (T)1;
    const T th0 = (T)t0, th1 = (T)t1, th2 = (T)t2, th3 = (T)t3;
    uint8_t *hp = hard + (size_t)ch * hstride;
    if constexpr (REAL) {
        // samples / max_power then sample * conj(prev) on real scalars: the product's sign (and
        // signed zero) decides; arctan2(+0, dr) is 0 or pi
        for (long k = 1 + lane; k < S; k += BS) {
            T sr = sp[k], pr = sp[k - 1];
            if (norm) {
                sr = sr / mx;
                pr = pr / mx;
            }
            const T ph = atan2((T)0, sr * pr);
            hp[k - 1] = ph < th0 ? 3 : ph < th1 ? 2 : ph < th2 ? 0 : ph < th3 ? 1 : 3;
        }
        return;
    }
    for (long k = 1 + lane; k < S; k += BS) {
        T sr = sp[2 * k], si = sp[2 * k + 1], pr = sp[2 * k - 2], pi = sp[2 * k - 1];
        if (norm) {
            const T a = (sr + si * rat) * scl, b = (si - sr * rat) * scl;
            const T c = (pr + pi * rat) * scl, d = (pi - pr * rat) * scl;
            sr = a; si = b; pr = c; pi = d;
        }
        // numpy scalar complex multiply sample * conj(prev), no FMA
        const T npi = -pi;
        const T dr = sr * pr - si * npi;
        const T di = sr * npi + si * pr;
        const T ph = atan2(di, dr);
        uint8_t s;
        if (ph < th0) s = 3;
        else if (ph < th1) s = 2;
        else if (ph < th2) s = 0;
        else if (ph < th3) s = 1;
        else s = 3;
        hp[k - 1] = s;
    }
}

// ----------------------------------------------------------------- host-side launchers
template <typename T>
void launch_extract(tetra_ctx *ctx, const void *yv, Lay ly, int C, long M, int sps, int step, void *symv, long smax,
                    int32_t *nsym, int32_t *bph, void *pwv = nullptr) {
    const T *y = (const T *)yv;
    T *sym = (T *)symv, *pw = (T *)pwv;
    PROF(ctx, "compat_extract");
    if (pw)   // latency mode: every |y|^2 first, in parallel
        hipLaunchKernelGGL(k_cabs2<T>, dim3(grid_for((size_t)C * M, 256)), dim3(256), 0, ctx->stream, y, ly, C, M, pw);
    if (pw && M / sps <= 3584)   // ... and each phase's pairwise sum leaf-parallel
        hipLaunchKernelGGL(k_extract_lat<T>, dim3(C), dim3(512), 0, ctx->stream, y, ly, C, M, sps, step, sym, smax, nsym,
                           bph, (const T *)pw);
    else
        hipLaunchKernelGGL(k_extract<T>, dim3(grid_for((size_t)16 * C, 256)), dim3(256), 0, ctx->stream, y, ly, C, M, sps,
                           step, sym, smax, nsym, bph, (const T *)pw);
}

template <typename T, bool REAL = false>
void launch_demod(tetra_ctx *ctx, const void *symv, long stride, int C, const int32_t *nsym, long S_all,
                  const double *thr, uint8_t *hard, long hstride) {
    const T *sym = (const T *)symv;
    PROF(ctx, "compat_demod");
    const bool few = C <= SB_MAXC;   // a few channels: a workgroup of 1024 per channel
    hipLaunchKernelGGL((few ? k_demod<T, 1024, REAL> : k_demod<T, 64, REAL>), dim3(C), dim3(few ? 1024 : 64), 0,
                       ctx->stream, sym, stride, C, nsym, S_all, thr[0], thr[1], thr[2], thr[3], hard, hstride);
}

}  // namespace

void compat_extract_decide(tetra_ctx *ctx, const tetra_compat_plan *P, int fmt, const void *y, Lay ly, int C, long M,
                           void *sym, int32_t *nsym, long smax, void *pw, uint8_t *hard) {
    if (fmt == TETRA_CF64) {
        launch_extract<double>(ctx, y, ly, C, M, P->sps, P->phase_step, sym, smax, nsym, nullptr, pw);
        launch_demod<double>(ctx, sym, smax, C, nsym, 0, P->thr, hard, smax);
    } else {
        launch_extract<float>(ctx, y, ly, C, M, P->sps, P->phase_step, sym, smax, nsym, nullptr, pw);
        launch_demod<float>(ctx, sym, smax, C, nsym, 0, P->thr, hard, smax);
    }
}

extern "C" {

int tetra_extract_symbols(tetra_ctx *ctx, const void *x, int fmt, size_t C, size_t N, int sps, int step, void *sym,
                          int32_t *nsym, int32_t *bestph, size_t smax) {
    if (!ctx || C == 0 || N == 0 || sps < 1 || step < 1) return tetra_fail(ctx, TETRA_E_INVALID, "bad extract args");
    if ((sps + step - 1) / step > 16) return tetra_fail(ctx, TETRA_E_INVALID, "more than 16 phases");
    const size_t es = compat_elem_size(ctx, fmt);
    if (!es) return TETRA_E_INVALID;
    Staging st(ctx);
    const void *xd = st.in(x, C * N * 2 * es);
    void *sd = st.out(sym, C * smax * 2 * es);
    int32_t *nd = (int32_t *)st.out(nsym, C * 4);
    int32_t *bd = bestph ? (int32_t *)st.out(bestph, C * 4) : nullptr;
    if (!xd || !sd || !nd) return st.finish();
    if (es == 8) launch_extract<double>(ctx, xd, row_major(N), (int)C, (long)N, sps, step, sd, (long)smax, nd, bd);
    else launch_extract<float>(ctx, xd, row_major(N), (int)C, (long)N, sps, step, sd, (long)smax, nd, bd);
    return st.finish();
}

int tetra_demod_dqpsk(tetra_ctx *ctx, const void *sym, int fmt, size_t C, size_t S, const double *thr4, uint8_t *hard) {
    if (!ctx || !thr4) return TETRA_E_INVALID;
    if (S < 2 || C == 0) return TETRA_OK;
    const bool real = fmt == TETRA_F32 || fmt == TETRA_F64;
    if (fmt != TETRA_CF32 && fmt != TETRA_CF64 && !real)
        return tetra_fail(ctx, TETRA_E_INVALID, "demod_dqpsk takes cf32/cf64/f32/f64");
    const size_t es = fmt == TETRA_CF64 || fmt == TETRA_F64 ? 8 : 4;
    Staging st(ctx);
    const void *sd = st.in(sym, C * S * (real ? 1 : 2) * es);
    uint8_t *hd = (uint8_t *)st.out(hard, C * (S - 1));
    if (!sd || !hd) return st.finish();
    const long s = (long)S;
    switch (fmt) {
    case TETRA_F64: launch_demod<double, true>(ctx, sd, s, (int)C, nullptr, s, thr4, hd, s - 1); break;
    case TETRA_F32: launch_demod<float, true>(ctx, sd, s, (int)C, nullptr, s, thr4, hd, s - 1); break;
    case TETRA_CF64: launch_demod<double>(ctx, sd, s, (int)C, nullptr, s, thr4, hd, s - 1); break;
    default: launch_demod<float>(ctx, sd, s, (int)C, nullptr, s, thr4, hd, s - 1); break;
    }
    return st.finish();
}

}  // extern "C"
