// compat_sos.h -- the pieces of the compat decimator (scipy sosfiltfilt, cheby1(8) -> 4 sections) that
// its sequential kernels (compat_demod.hip) and its time-tiled kernels (compat_tiled.hip) share: the
// row layouts, the one-section DF-II-T step in scipy's operation order, and the banked lane mapping.
#pragma once
#include "common.h"

namespace {

// Strided view of complex rows: element (ch, n) real part at base[off(ch, n)], imag at +1.
struct Lay {
    size_t s_grp, s_n, s_lane;
    __host__ __device__ size_t off(int ch, long n) const {
        return (size_t)(ch >> 5) * s_grp + (size_t)n * s_n + (size_t)(ch & 31) * s_lane;
    }
};
static Lay row_major(long len) { return Lay{(size_t)64 * len, 2, (size_t)2 * len}; }
static Lay grouped(long len) { return Lay{(size_t)64 * len, 64, 2}; }
static size_t grouped_elems(int C, long len) { return (size_t)((C + 31) / 32) * 64 * (size_t)len; }

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
