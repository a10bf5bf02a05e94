// compat_sos.h -- what the units of the compat chain share: the row layouts, the time-blocked limits
// and the stage entry points tetra_demod_compat (compat_demod.hip) strings together; then the pieces
// of the decimator (sosfiltfilt, 4 sections) common to compat_decimate.hip and compat_tiled.hip: the
// one-section DF-II-T step in scipy's operation order and the banked lane mapping.
#pragma once
#include "common.h"

// Strided view of complex rows: element (ch, n) real part at base[off(ch, n)], imag at +1.
struct Lay {
    size_t s_grp, s_n, s_lane;
    __host__ __device__ size_t off(int ch, long n) const {
        return (size_t)(ch >> 5) * s_grp + (size_t)n * s_n + (size_t)(ch & 31) * s_lane;
    }
};
inline Lay row_major(long len) { return Lay{(size_t)64 * len, 2, (size_t)2 * len}; }
inline Lay grouped(long len) { return Lay{(size_t)64 * len, 64, 2}; }
inline size_t grouped_elems(int C, long len) { return (size_t)((C + 31) / 32) * 64 * (size_t)len; }
inline long ceil_div(long a, long b) { return (a + b - 1) / b; }
// out = P P, row-major n x n (n <= 8, out may be P): every product summed in k order without FMA
inline void mat_square(const double *P, double *out, int n) {
    double t[64];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double acc = 0.0;
            for (int k = 0; k < n; ++k) acc = acc + P[i * n + k] * P[k * n + j];
            t[i * n + j] = acc;
        }
    for (int i = 0; i < n * n; ++i) out[i] = t[i];
}

// The time-blocked (latency mode) decimator's and filtfilt's tiles, and the shapes they serve.
constexpr int SB_B = 256;        // decimator: samples per tile
constexpr int SB_MAXT = 1024;    // tiles per stream (one scan workgroup): L <= 262144
constexpr int SB_NPOW = 10;      // Phi^(2^r), r < SB_NPOW: covers SB_MAXT tiles
constexpr int SB_MAXC = 64;      // channels up to which tetra_demod_compat takes this path
constexpr int SB_MAXQ = 16;      // decimation factors up to which it does
constexpr int LB_B = 128;        // filtfilt: samples per tile
constexpr int LB_NS = 4;         // states (butter(4): 5 taps)
inline bool blocked_fits(int C, long N, int q) {
    return C >= 1 && C <= SB_MAXC && q >= 2 && q <= SB_MAXQ && N > 27 && (N + 54 + SB_B - 1) / SB_B <= SB_MAXT;
}
inline bool lf_blocked_fits(int C, long M, int ntaps) {
    return C >= 1 && C <= SB_MAXC && ntaps == LB_NS + 1 && (M + 6 * ntaps + LB_B - 1) / LB_B <= SB_MAXT;
}

// The compat path's sample formats: the element size of cf32 / cf64, or 0 with the error set.
inline size_t compat_elem_size(tetra_ctx *ctx, int fmt) {
    if (fmt == TETRA_CF32 || fmt == TETRA_CF64) return fmt == TETRA_CF64 ? 8 : 4;
    tetra_fail(ctx, TETRA_E_INVALID, "compat path takes cf32/cf64");
    return 0;
}
int check_plan(tetra_ctx *ctx, const tetra_compat_plan *P);   // compat_demod.hip

// Stage entry points: samples as untyped pointers with their format (TETRA_CF32 / CF64), which each
// unit resolves to float / double once.  compat_decimate.hip (DEC_TILED: cf32 only):
enum DecForm { DEC_SEQUENTIAL, DEC_BLOCKED, DEC_TILED };
int compat_decimate(tetra_ctx *ctx, const tetra_compat_plan *P, int fmt, DecForm form, const void *x, int C, long N,
                    void *out, Lay lo);
void blocked_table(const double *coef /*[24] sos rows*/, double *tab /*[SB_NPOW * 64]*/);
// compat_filtfilt.hip: frequency_shift of the rows with mixon set (all when it is null), and filtfilt
// with that mixer inside the recursion, after k_mix (LF_PREMIX: every row mixed) or time-blocked.
enum LfForm { LF_SEQUENTIAL, LF_PREMIX, LF_BLOCKED };
int launch_mix(tetra_ctx *ctx, int fmt, const void *x, Lay lx, int C, long N, const double *mixc,
                const uint8_t *mixon, double fs, double *out, Lay lo);
int compat_filtfilt(tetra_ctx *ctx, const tetra_compat_plan *P, int fmt, LfForm form, const void *x, Lay lx, int C,
                    long M, const double *mixc, const uint8_t *mixon, double *out, Lay lo);
void lfilter_table(const double *bcoef, const double *acoef, double *tab /*[SB_NPOW * 16]*/);
// compat_symbols.hip: extract_symbols (over the |y|^2 rows pw when given), then demodulate_dqpsk.
void compat_extract_decide(tetra_ctx *ctx, const tetra_compat_plan *P, int fmt, const void *y, Lay ly, int C, long M,
                           void *sym, int32_t *nsym, long smax, void *pw, uint8_t *hard);

// The decimator's coefficients in precision T (24 sos words, 8 of sosfilt_zi) to `coef`, sos to dc
template <typename T>
int upload_sos_coef(tetra_ctx *ctx, const tetra_compat_plan *P, T *coef, double *dc = nullptr) {
    T hc[32];
    for (int i = 0; i < 24; ++i) hc[i] = std::is_same<T, float>::value ? (T)P->sos_f32[i] : (T)P->sos_f64[i];
    for (int i = 0; i < 8; ++i) hc[24 + i] = std::is_same<T, float>::value ? (T)P->zi_f32[i] : (T)P->zi_f64[i];
    for (int i = 0; dc && i < 24; ++i) dc[i] = (double)hc[i];
    HIP_TRY(ctx, hipMemcpyAsync(coef, hc, sizeof hc, hipMemcpyHostToDevice, ctx->stream));
    return TETRA_OK;
}

namespace {

constexpr int NSEC = 4;   // decimate's cheby1(8) -> 4 second-order sections

template <typename T>
struct Biquad {
    T b0, b1, b2, a1, a2, z0, z1;
    __device__ __forceinline__ T step(T x) {   // scipy _sosfilt, one section
        const T xn = b0 * x + z0;
        z0 = (b1 * x - a1 * xn) + z1;
        z1 = b2 * x - a2 * xn;
        return xn;
    }
};

// fp32: the same operations, paired -- (b1 x, b2 x) and (a1 xn, a2 xn) are each one v_pk_mul_f32
// (x and xn broadcast by op_sel_hi) and the two differences one v_pk_add_f32 (the product negated
// by neg_lo/neg_hi: a - b and a + (-b) are the same IEEE operation), so a section's tick is 6 VALU
// instead of 9.  Every product and sum is the scalar one, rounded once: bit-identical.
typedef float pkf2 __attribute__((ext_vector_type(2)));
template <>
struct Biquad<float> {
    pkf2 b12, a12;
    float b0, z0, z1;
    __device__ __forceinline__ Biquad(float b0_, float b1, float b2, float a1, float a2, float z0_, float z1_)
        : b12{b1, b2}, a12{a1, a2}, b0(b0_), z0(z0_), z1(z1_) {}
    __device__ __forceinline__ float step(float x) {
        const float m0 = b0 * x;
        const pkf2 p1 = b12 * pkf2{x, x};
        const float xn = m0 + z0;
        const pkf2 p3 = p1 - a12 * pkf2{xn, xn};
        z0 = p3.x + z1;
        z1 = p3.y;
        return xn;
    }
};

template <typename T>
__device__ __forceinline__ Biquad<T> load_section(const T *sos, const T *zi, int s, T x0) {
    return Biquad<T>{sos[6 * s], sos[6 * s + 1], sos[6 * s + 2], sos[6 * s + 4], sos[6 * s + 5], zi[2 * s] * x0,
                     zi[2 * s + 1] * x0};
}

constexpr int SOS_PD = 2;   // banked decimator passes: input batches in flight

// ------------------------------------------------------------------ fp32 decimator, banked lanes
// The kernels above are bound by the texture data path (TD ~95 % busy, r01 PMC): the four
// section lanes of a stream, and for the forward pass both components of a channel, load the same
// 16 bytes, so every load instruction returns 1 KiB for 128-256 useful bytes.  Here the section
// is the DPP bank instead of the low lane bits:
//   lane = 16 row + 4 sec + s,   stream g = 16 wave + 4 row + s   (g = 2 ch + comp)
// The section chain moves one bank right per tick (row_shr:4), and the 4 lanes of a stream load 4
// DIFFERENT 16-byte chunks of its input window; section 0 (bank 0) takes the tick's sample from
// the lane of bank j with row_shl:4j under bank_mask 1 -- the same DPP move that replaces the
// section-0 select, so a tick is 2 DPP moves + the 9-operation biquad.  Arithmetic per section and
// sample is unchanged (bit-identical to the kernels above and to scipy's _sosfilt).
template <int CTRL, int BANKS, bool BC>
__device__ __forceinline__ float dppf(float old, float src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old),
                                                                 __builtin_bit_cast(int, src), CTRL, 0xf, BANKS, BC));
}
// section 0 takes src of bank j (compile time); the other banks keep `left`
template <int J>
__device__ __forceinline__ float bank0_from(float left, float src) {
    if constexpr (J == 0) return dppf<0xE4, 0x1, false>(left, src);   // quad_perm identity
    else return dppf<0x100 + 4 * J, 0x1, false>(left, src);            // row_shl:4J
}
__device__ __forceinline__ float from_left_bank(float y) { return dppf<0x114, 0xf, true>(0.f, y); }   // row_shr:4

// 4-byte aligned 16-byte load (the imaginary stream's window starts one float into a complex pair)
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

struct BankLane {
    int sec, g, ch, comp;
    bool own, st;
    __device__ BankLane(int C) {
        const int lane = threadIdx.x & 63, w = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
        sec = (lane >> 2) & 3;
        g = 16 * w + 4 * (lane >> 4) + (lane & 3);
        ch = min(g >> 1, C - 1);   // tail lanes shadow the last stream and store nothing
        comp = g & 1;
        own = (g >> 1) < C;
        st = own && sec == 3;
    }
};

}  // namespace
