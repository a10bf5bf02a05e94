// etsi_coding.h -- the EN 300 392-2 channel-coding constants the lower-MAC units share (etsi_lmac.hip,
// etsi_quality.hip, etsi_traffic.hip): block kinds, burst patterns, the puncturer, the CRC-16 and the scrambler as
// linear tables.  Each unit gets its own copy (the unit's anonymous namespace).
#pragma once
#include "common.h"

namespace {

constexpr int ETSI_MAXB = 8;   // bursts per channel chunk
constexpr int ETSI_MAXJ = 16;   // coded blocks per channel chunk (2 per burst)

struct KindP { int K, a, n2, n1; };
__host__ __device__ constexpr KindP kind_params(int kind) {
    return kind == 0 ? KindP{432, 103, 288, 268} : kind == 1 ? KindP{216, 101, 144, 124} : KindP{120, 11, 80, 60};
}

// training/tail patterns (EN 300 392-2 §9.4.4.3), LSB-first words
__host__ __device__ constexpr uint64_t packb(const int *p, int n) {
    uint64_t w = 0;
    for (int j = 0; j < n; ++j) w |= (uint64_t)p[j] << j;
    return w;
}
constexpr int QB[22] = {1, 0, 1, 1, 0, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0, 1, 1, 0, 1};
constexpr int NB[22] = {1, 1, 0, 1, 0, 0, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1, 0, 0};
constexpr int PB[22] = {0, 1, 1, 1, 1, 0, 1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 1, 1, 1, 0, 0};
constexpr int YB[38] = {1, 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 1, 0, 0, 1, 1, 1,
                        0, 1, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 1};
constexpr uint64_t W_HEAD = packb(QB + 10, 12), W_TAIL = packb(QB, 10), W_N = packb(NB, 22), W_P = packb(PB, 22),
                   W_Y = packb(YB, 38);

__host__ __device__ constexpr int punct_index(int j1) {   // rate 2/3, t=3, P=(1,2,5); 1-based
    const int g = (j1 - 1) / 3;
    const int r = j1 - 3 * g;
    return 8 * g + (r == 1 ? 1 : r == 2 ? 2 : 5);
}

// CRC-16 register as a linear function of the bits (GF(2)): reg(L bits) = INIT[L] ^ XOR over
// 1-bits at distance d from the end of T[d].  Lets the serial traceback, which emits bits last
// to first, check the CRC on the fly instead of a second serial pass.
struct CrcTab {
    uint32_t t[288];   // dwords: read with wave-uniform scalar loads
    uint32_t init[289];
};
constexpr uint32_t crc_step(uint32_t r) { return ((r & 0x8000u) ? ((r << 1) ^ 0x1021u) : (r << 1)) & 0xFFFFu; }
constexpr CrcTab make_crc_tab() {
    CrcTab c{};
    uint32_t r = crc_step(0x8000u);
    for (int d = 0; d < 288; ++d) { c.t[d] = r; r = crc_step(r); }
    uint32_t s = 0xFFFFu;
    for (int L = 0; L <= 288; ++L) { c.init[L] = s; s = crc_step(s); }
    return c;
}
__constant__ CrcTab CRC_TAB = make_crc_tab();

// The scrambler (EN 300 392-2 §8.2.5) is linear over GF(2): with x[0..31] the init's bits and
// x[n + 32] = XOR over the taps t of x[n + t], its output bit n is x[n + 32] = parity(init &
// SCR_MASK.w[n]).  The table lets lanes form the 432 bits independently where a register steps.
constexpr uint32_t SCR_TAPS = (1u << 0) | (1u << 6) | (1u << 9) | (1u << 10) | (1u << 16) | (1u << 20) | (1u << 21) |
                              (1u << 22) | (1u << 24) | (1u << 25) | (1u << 27) | (1u << 28) | (1u << 30) | (1u << 31);
struct ScrMask {
    alignas(16) uint32_t w[432];
};
constexpr ScrMask make_scr_mask() {
    ScrMask m{};
    uint32_t x[32 + 432] = {};
    for (int i = 0; i < 32; ++i) x[i] = 1u << i;
    for (int n = 0; n < 432; ++n) {
        uint32_t v = 0;
        for (int t = 0; t < 32; ++t)
            if ((SCR_TAPS >> t) & 1u) v ^= x[n + t];
        x[n + 32] = v;
        m.w[n] = v;
    }
    return m;
}
__constant__ ScrMask SCR_MASK = make_scr_mask();

// the post-passes over the rows a lower-MAC call read (etsi_quality.hip, etsi_traffic.hip)
__device__ __forceinline__ uint32_t load_u32(const void *p) {   // any alignment
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// whether burst b of the row lies in it: kind 0..2 and row bits [origin + start, + 510) inside 2 stride
__device__ __forceinline__ bool burst_ok(const int32_t *bu, int b, long origin, long row_bits, long &p0, int &kind) {
    kind = bu[2 * b + 1];
    p0 = origin + (long)bu[2 * b];
    return kind >= 0 && kind <= 2 && p0 >= 0 && p0 + 510 <= row_bits;
}

}  // namespace
