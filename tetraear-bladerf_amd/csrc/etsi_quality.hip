// etsi_quality.hip -- link quality of the ETSI chain's decoded bursts and blocks on gfx950
// (tetra_etsi_link_quality): a post-pass over the rows the lower MAC read and the records it wrote,
// restated in tests/_etsi_quality_model.py.
//
//   k_etsi_quality  one workgroup per row, 16 lanes per block (group j on block j): a CRC-good block's
//               type-1 bytes are packed into an LDS bit row (a lane 32 of them), the CRC-16 taken from
//               the linear table as an XOR reduction over the group, and each lane then re-encodes
//               four type-5 bits at a time straight from that row -- inverse interleaver, puncturer,
//               the mother code as a parity over a 5-bit window, the scrambler bit as a parity of the
//               cell's init -- and compares them with the four soft bytes of one dword load.  The four
//               sums are reduced over the group.  Group 8 + b forms burst b's record first (a row
//               seldom has more than 8 blocks, so those groups are otherwise idle): its head, training
//               and tail bits against the patterns, and |soft| over its 510 bits.  A group's LDS row is
//               its own and a group lies in one wave: no workgroup barrier, and a wave with neither a
//               block nor a burst ends at once.
#include "common.h"
#include "etsi_coding.h"

namespace {

constexpr int LQ_LANES = 16;               // lanes per block / burst
constexpr int LQ_BLOCK = LQ_LANES * ETSI_MAXJ;   // one row per workgroup
constexpr int LQ_ROW = 17;                 // LDS dwords per group: a zero dword, 288 type-2 bits, zeros; odd
constexpr int NQ = TETRA_LQ_FIELDS;
static_assert(TETRA_LQ_FIELDS == 4 && TETRA_ETSI_MAXB == ETSI_MAXB && TETRA_ETSI_MAXJ == ETSI_MAXJ, "record layout");

// a^-1 mod K: type-5 position k - 1 = a i mod K holds type-3 bit i = ainv (k - 1) mod K (0 -> K)
constexpr int inv_mod(int a, int K) {
    for (int x = 1; x < K; ++x)
        if ((long)a * x % K == 1) return x;
    return 0;
}
constexpr int AINV[3] = {inv_mod(103, 432), inv_mod(101, 216), inv_mod(11, 120)};
static_assert(AINV[0] != 0 && AINV[1] != 0 && AINV[2] != 0,"interleaver multipliers are units");

// taps of the rate-1/4 mother code's generator g on the window (bit 4 = the step's bit, bit 4 - d the
// bit d steps earlier): G1 = 1 + D + D^4, G2 = 1 + D^2 + D^3 + D^4, G3 = 1 + D + D^2 + D^4, G4 = 1 + D + D^3 + D^4
__device__ __forceinline__ uint32_t gen_taps(int g) { return g == 0 ? 0x19u : g == 1 ? 0x17u : g == 2 ? 0x1Du : 0x1Bu; }

// the puncturer in the form the kernel uses it (checked against punct_index for every type-3 bit)
constexpr bool punct_form_ok() {
    for (int i = 1; i <= 432; ++i) {
        const int t = i - 1, t3 = t / 3, r = t - 3 * t3, mi = punct_index(i) - 1;
        if ((mi >> 2) != 2 * t3 + (r == 2) || (mi & 3) != (r == 1)) return false;
    }
    return true;
}
static_assert(punct_form_ok(), "puncturer");

__device__ __forceinline__ uint32_t group_xor(uint32_t v) {
#pragma unroll
    for (int m = LQ_LANES / 2; m >= 1; m >>= 1) v ^= (uint32_t)__shfl_xor((int)v, m, LQ_LANES);
    return v;
}
__device__ __forceinline__ uint32_t group_sum(uint32_t v) {
#pragma unroll
    for (int m = LQ_LANES / 2; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, LQ_LANES);
    return v;
}

__device__ __forceinline__ int hard_bit(const uint8_t *hrow, long p) {   // as the burst scan reads it
    const uint32_t h = hrow[p >> 1];
    return (int)((p & 1) ? h & 1u : (h >> 1) & 1u);
}

// Burst b of a row by one group of 16 lanes: its record to o[0..3].
__device__ __forceinline__ void score_burst(const int8_t *__restrict__ srow, const uint8_t *__restrict__ hrow,
                                            const int32_t *__restrict__ bu, int b, long origin, long row_bits, int l,
                                            int32_t *__restrict__ o) {
    long p0;
    int bkind;
    if (!burst_ok(bu, b, origin, row_bits, p0, bkind)) {
        if (l < NQ) o[l] = -1;
        return;
    }
    // 22 head + tail bits, then 22 (n, p) or 38 (y) training bits: bit e of lane l is l + 16 e
    const int ntr = bkind == 2 ? 38 : 22;
    const uint64_t wtr = bkind == 2 ? W_Y : bkind == 1 ? W_P : W_N;
    const int tr0 = bkind == 2 ? 214 : 244;
    uint32_t errs = 0;   // TERR | HERR << 16
    for (int e = l; e < 22 + ntr; e += LQ_LANES) {
        long p;
        uint32_t want, sh;
        if (e < 12) { p = p0 + e; want = (uint32_t)(W_HEAD >> e) & 1u; sh = 16; }
        else if (e < 22) { p = p0 + 500 + (e - 12); want = (uint32_t)(W_TAIL >> (e - 12)) & 1u; sh = 16; }
        else { p = p0 + tr0 + (e - 22); want = (uint32_t)(wtr >> (e - 22)) & 1u; sh = 0; }
        errs += (uint32_t)(hard_bit(hrow, p) != (int)want) << sh;
    }
    // |soft| over the 510 bits: lane l takes bytes 32 l .. 32 l + 31, the last lane 30
    uint32_t wsum = 0, nsat = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = 32 * l + 4 * u;
        if (i + 4 <= 510) {
            const uint32_t sv = load_u32(srow + p0 + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int s = (int8_t)(sv >> (8 * k));
                const uint32_t mag = (uint32_t)(s < 0 ? -s : s);
                wsum += mag;
                nsat += mag >= 127;
            }
        } else if (i < 510) {   // bytes 508, 509
            for (int k = 0; k < 510 - i; ++k) {
                const int s = srow[p0 + i + k];
                const uint32_t mag = (uint32_t)(s < 0 ? -s : s);
                wsum += mag;
                nsat += mag >= 127;
            }
        }
    }
    errs = group_sum(errs);
    wsum = group_sum(wsum);
    nsat = group_sum(nsat);
    if (l == 0) {
        o[TETRA_BQ_TERR] = (int32_t)(errs & 0xFFFFu);
        o[TETRA_BQ_HERR] = (int32_t)(errs >> 16);
        o[TETRA_BQ_WSUM] = (int32_t)wsum;
        o[TETRA_BQ_NSAT] = (int32_t)nsat;
    }
}

__global__ __launch_bounds__(LQ_BLOCK) void k_etsi_quality(
    const int8_t *__restrict__ softbits, const uint8_t *__restrict__ hard, int C, long stride, int origin, int G,
    const uint32_t *__restrict__ cell_init, const int32_t *__restrict__ nburst, const int32_t *__restrict__ bursts,
    const int32_t *__restrict__ nblock, const int32_t *__restrict__ blocks, const uint8_t *__restrict__ type1,
    int32_t *__restrict__ bq, int32_t *__restrict__ kq) {
    __shared__ uint32_t rows[ETSI_MAXJ * LQ_ROW];
    const int tid = threadIdx.x, j = tid / LQ_LANES, l = tid % LQ_LANES;
    const long ch = blockIdx.x;   // the grid is C workgroups
    const long row_bits = 2 * stride;
    const int8_t *srow = softbits + ch * row_bits;
    const uint8_t *hrow = hard + ch * stride;
    const int32_t *bu = bursts + ch * ETSI_MAXB * 2;
    const int nb = min(max(nburst[ch], 0), ETSI_MAXB), nk = min(max(nblock[ch], 0), ETSI_MAXJ);
    const int g0 = j & ~3;   // the wave's first group (wave-uniform): blocks g0 .. g0 + 3, bursts g0 - 8 .. g0 - 5
    if (g0 >= nk && (g0 < ETSI_MAXB || g0 - ETSI_MAXB >= nb)) return;
    uint32_t *row = rows + j * LQ_ROW;

    // ---- burst j - 8 (groups 8..15)
    if (j >= ETSI_MAXB && j - ETSI_MAXB < nb)
        score_burst(srow, hrow, bu, j - ETSI_MAXB, origin, row_bits, l, bq + ((size_t)ch * ETSI_MAXB + j - ETSI_MAXB) * NQ);

    // ---- block j: what it is and where its soft bits lie (group-uniform)
    const size_t cj = (size_t)ch * ETSI_MAXJ + j;
    int state = 0;   // 0 no record, 1 all -1, 2 CRC-bad, 3 scored
    int kind = 0;
    long base = 0;
    if (j < nk) {
        kind = blocks[4 * cj];
        const int crc = blocks[4 * cj + 1], b = blocks[4 * cj + 2], blk = blocks[4 * cj + 3];
        state = 1;
        long p0;
        int bkind;
        // a block that names no live burst, or a kind / index pair no burst carries, reads as its burst invalid
        if (kind >= 0 && kind <= 2 && b >= 0 && b < nb && (blk == 0 || (blk == 1 && kind == 1)) &&
            burst_ok(bu, b, origin, row_bits, p0, bkind)) {
            base = p0 + (blk == 1 ? 282 : kind == 2 ? 94 : 14);
            state = crc != 0 ? 3 : 2;
        }
    }
    const KindP P = kind_params(kind);
    uint32_t raw = 0;   // type-2 bits 32 l .. 32 l + 31, LSB first
    if (state == 3) {
        const uint8_t *t = type1 + cj * 268;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = 32 * l + 4 * u;
            const uint32_t v = i < P.n1 ? load_u32(t + i) : 0u;   // n1 is a multiple of 4
            raw |= (((v & 0x01010101u) * 0x01020408u) >> 24) << (4 * u);
        }
        // CRC-16 over the n1 bits: bit t sits n1 - 1 - t from the end
        uint32_t x = 0;
#pragma unroll 8
        for (int u = 0; u < 32; ++u) {
            const int d = P.n1 - 1 - (32 * l + u);
            x ^= CRC_TAB.t[max(d, 0)] & (0u - ((raw >> u) & 1u));   // raw is 0 from bit n1 on
        }
        const uint32_t crc = (group_xor(x) ^ CRC_TAB.init[P.n1] ^ 0xFFFFu) & 0xFFFFu;
        const uint32_t rev = __brev(crc) >> 16;   // bit k = CRC bit 15 - k: type-2 bit n1 + k
        const int q = P.n1 >> 5, sh = P.n1 & 31;
        if (l == q) raw |= rev << sh;
        if (l == q + 1 && sh > 16) raw |= rev >> (32 - sh);
    }
    row[1 + l] = raw;   // type-2 bit s at row bit 32 + s; the four tail bits and everything past them 0
    if (l == 0) row[0] = 0;
    // the row is the group's own and the group lies in one wave: wave-scope ordering is enough
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    if (state == 3) {
        const int ainv = AINV[kind];
        const uint32_t init = kind == 2 ? 3u : cell_init[ch / G];
        uint32_t cnt = 0, wgt = 0;   // NERR | NZERO << 16, WERR | WSUM << 16 (each at most 432 x 128 < 2^16)
        // the type-3 index of the lane's first position, and its advance per step of 64 positions: the
        // interleaver's inverse by additions, two divisions a block instead of one a step
        int i3d = ainv * 4 * l % P.K;
        const int adv = ainv * 4 * LQ_LANES % P.K;
        for (int d = l; 4 * d < P.K; d += LQ_LANES) {
            const int i5 = 4 * d;   // K and SCH/F's gap at 216 are multiples of 4
            const uint32_t sv = load_u32(srow + base + i5 + (kind == 0 && i5 >= 216 ? 52 : 0));
            const uint4 mk = *reinterpret_cast<const uint4 *>(&SCR_MASK.w[i5]);
            const uint32_t scr = ((uint32_t)__popc(init & mk.x) & 1u) | (((uint32_t)__popc(init & mk.y) & 1u) << 1) |
                                 (((uint32_t)__popc(init & mk.z) & 1u) << 2) | (((uint32_t)__popc(init & mk.w) & 1u) << 3);
            int i3 = i3d;
            i3d += adv;
            if (i3d >= P.K) i3d -= P.K;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                // type-3 bit i = 3 t3 + r + 1 is mother bit 8 t3 + (0, 1, 4)[r] (punct_index): trellis step
                // 2 t3 + (r == 2), generator G2 for r == 1, else G1
                const int t = (i3 == 0 ? P.K : i3) - 1, t3 = t / 3, r = t - 3 * t3;
                const int pos = 2 * t3 + (r == 2) + 28;   // the window's first row bit
                const uint32_t win = __builtin_amdgcn_alignbit(row[(pos >> 5) + 1], row[pos >> 5], (uint32_t)(pos & 31));
                const uint32_t c = ((uint32_t)__popc(win & (r == 1 ? gen_taps(1) : gen_taps(0))) ^ (scr >> u)) & 1u;
                const int s = (int8_t)(sv >> (8 * u));
                const uint32_t mag = (uint32_t)(s < 0 ? -s : s);
                const uint32_t bad = s != 0 && (uint32_t)(s < 0) != c;
                cnt += bad | ((uint32_t)(s == 0) << 16);
                wgt += (bad ? mag : 0u) | (mag << 16);
                i3 += ainv;
                if (i3 >= P.K) i3 -= P.K;
            }
        }
        cnt = group_sum(cnt);
        wgt = group_sum(wgt);
        if (l == 0) {
            int32_t *o = kq + cj * NQ;
            o[TETRA_LQ_NERR] = (int32_t)(cnt & 0xFFFFu);
            o[TETRA_LQ_WERR] = (int32_t)(wgt & 0xFFFFu);
            o[TETRA_LQ_WSUM] = (int32_t)(wgt >> 16);
            o[TETRA_LQ_NZERO] = (int32_t)(cnt >> 16);
        }
    } else if (state != 0 && l < NQ) {
        kq[cj * NQ + l] = l == 0 || state == 1 ? -1 : 0;
    }
}

}  // namespace

extern "C" int tetra_etsi_link_quality(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, size_t C,
                                       size_t stride, int32_t origin_bits, size_t G, const uint32_t *cell_init,
                                       const int32_t *nburst, const int32_t *bursts, const int32_t *nblock,
                                       const int32_t *blocks, const uint8_t *type1, int32_t *bq, int32_t *kq) {
    if (!ctx) return TETRA_E_INVALID;
    if (C == 0 || stride == 0 || !softbits || !hard || !cell_init || !nburst || !bursts || !nblock || !blocks ||
        !type1 || !bq || !kq)
        return tetra_fail(ctx, TETRA_E_INVALID, "tetra_etsi_link_quality: C > 0, stride > 0 and every array");
    if (G < 1 || C % G != 0 || origin_bits < 0)
        return tetra_fail(ctx, TETRA_E_INVALID,
                          "tetra_etsi_link_quality: G >= 1 rows per cell dividing C and origin_bits >= 0 (C %zu, G %zu, "
                          "origin_bits %d)", C, G, (int)origin_bits);
    if (C > ((size_t)1 << 24) || G > ((size_t)1 << 24) || stride > ((size_t)1 << 28))
        return tetra_fail(ctx, TETRA_E_INVALID, "too many rows or too long a row for one tetra_etsi_link_quality call");
    Staging st(ctx);
    // the three small host arrays travel as one staged input (six staged inputs in all)
    Staging::Part small[] = {{cell_init, C / G}, {nburst, C}, {nblock, C}};
    if (!st.pack(small)) return st.finish();
    const uint32_t *ci = (const uint32_t *)small[0].p;
    const int32_t *nb = (const int32_t *)small[1].p, *nk = (const int32_t *)small[2].p;
    const int8_t *sb = (const int8_t *)st.in(softbits, C * stride * 2);
    const uint8_t *hd = (const uint8_t *)st.in(hard, C * stride);
    const int32_t *bu = (const int32_t *)st.in(bursts, C * ETSI_MAXB * 2 * 4);
    const int32_t *bk = (const int32_t *)st.in(blocks, C * ETSI_MAXJ * 4 * 4);
    const uint8_t *t1 = (const uint8_t *)st.in(type1, C * ETSI_MAXJ * 268);
    // in/out: the records past nburst / nblock keep the caller's contents in host memory too
    int32_t *bo = (int32_t *)st.inout(bq, C * ETSI_MAXB * NQ * 4);
    int32_t *ko = (int32_t *)st.inout(kq, C * ETSI_MAXJ * NQ * 4);
    if (!sb || !hd || !bu || !bk || !t1 || !bo || !ko) return st.finish();
    {
        PROF(ctx, "etsi_quality");
        hipLaunchKernelGGL(k_etsi_quality, dim3((unsigned)C), dim3(LQ_BLOCK), 0, ctx->stream, sb, hd, (int)C,
                           (long)stride, (int)origin_bits, (int)G, ci, nb, bu, nk, bk, t1, bo, ko);
    }
    return st.finish();
}
