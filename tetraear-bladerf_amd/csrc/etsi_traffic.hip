// etsi_traffic.hip -- the ETSI chain's traffic slots as descrambled type-4 soft bits on gfx950
// (tetra_etsi_traffic): a post-pass over the rows the lower MAC read and the records it (and the MAC
// call) wrote, restated in tests/_etsi_traffic_model.py.
//
//   k_etsi_traffic  one workgroup per row, 32 lanes per burst (group b on burst b, two groups a wave):
//               the burst's class comes from the row's block records, one a lane, with a ballot over
//               the group; a FULL or HALF burst's block fields are then copied out descrambled -- a
//               lane takes output dwords l, l + 32, l + 64, l + 96 of the 108 (54), each one any-alignment
//               dword load of four soft bytes, four scrambler bits as parities of the cell's init
//               against one uint4 of SCR_MASK, the byte-wise negation (-128 -> 127) in registers and
//               one any-alignment dword store -- and |tch| and the zeros are summed over the group.
//               No LDS, no atomics; a wave with no burst ends at once.
#include "common.h"
#include "etsi_coding.h"

namespace {

constexpr int TQ_LANES = 32;                     // lanes per burst
constexpr int TQ_BLOCK = TQ_LANES * ETSI_MAXB;   // one row per workgroup
constexpr int NT = TETRA_TQ_FIELDS;
static_assert(TETRA_TQ_FIELDS == 4 && TETRA_ETSI_MAXB == ETSI_MAXB && TETRA_ETSI_MAXJ == ETSI_MAXJ &&
              TETRA_TCH_BITS == 432 && ETSI_MAXJ <= TQ_LANES && TETRA_TCH_BITS % 4 == 0, "record layout");

// a dword store at any alignment, load_u32's counterpart: gfx950 takes global dword accesses at any byte
// address, so a tch base that is not dword aligned needs no path of its own
__device__ __forceinline__ void store_u32(void *p, uint32_t v) { __builtin_memcpy(p, &v, 4); }

__device__ __forceinline__ uint32_t group_sum(uint32_t v) {
#pragma unroll
    for (int m = TQ_LANES / 2; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, TQ_LANES);
    return v;
}

__global__ __launch_bounds__(TQ_BLOCK) void k_etsi_traffic(
    const int8_t *__restrict__ softbits, int C, long stride, int origin, int G, const uint32_t *__restrict__ cell_init,
    const int32_t *__restrict__ nburst, const int32_t *__restrict__ bursts, const int32_t *__restrict__ nblock,
    const int32_t *__restrict__ blocks, const int32_t *__restrict__ slots, const int32_t *__restrict__ keep,
    int32_t *__restrict__ tq, int8_t *__restrict__ tch) {
    const int tid = threadIdx.x, b = tid / TQ_LANES, l = tid % TQ_LANES;
    const long ch = blockIdx.x;   // the grid is C workgroups
    const int nb = min(max(nburst[ch], 0), ETSI_MAXB), nk = min(max(nblock[ch], 0), ETSI_MAXJ);
    if ((b & ~1) >= nb) return;   // the wave's first burst (wave-uniform): bursts b & ~1 and that + 1
    const long row_bits = 2 * stride;
    const int8_t *srow = softbits + ch * row_bits;
    const int32_t *bu = bursts + ch * ETSI_MAXB * 2;
    const size_t cb = (size_t)ch * ETSI_MAXB + b;

    // ---- the burst (group-uniform)
    const bool live = b < nb;
    long p0 = 0;
    int bkind = 0;
    const bool valid = live && burst_ok(bu, b, origin, row_bits, p0, bkind);
    // ---- the row's block records, one a lane: does record l name this burst's block 0 / block 1 as CRC-good
    uint32_t hit = 0;
    if (valid && l < nk) {
        const int32_t *r = blocks + ((size_t)ch * ETSI_MAXJ + l) * 4;
        if (r[0] == bkind && r[1] != 0 && r[2] == b) hit = r[3] == 0 ? 1u : r[3] == 1 ? 2u : 0u;
    }
    // every lane of the wave is here: the group's half of the two ballots
    const int half = (tid & 32) ? 32 : 0;
    const bool g0 = ((uint32_t)(__ballot((hit & 1u) != 0) >> half)) != 0;
    const bool g1 = ((uint32_t)(__ballot((hit & 2u) != 0) >> half)) != 0;
    if (!live) return;
    int32_t *o = tq + cb * NT;
    if (!valid) {
        if (l < NT) o[l] = -1;
        return;
    }
    int cls;
    if (keep && keep[cb] == 0) cls = TETRA_TCH_NONE;
    else if (bkind == 2) cls = TETRA_TCH_NONE;
    else if (slots && slots[cb * TETRA_SLOT_FIELDS + TETRA_SLOT_FN] == 18) cls = TETRA_TCH_CONTROL;
    else if (bkind == 0) cls = g0 ? TETRA_TCH_CONTROL : TETRA_TCH_FULL;
    else cls = g0 && g1 ? TETRA_TCH_CONTROL : g0 ? TETRA_TCH_HALF : TETRA_TCH_LOST;
    if (cls != TETRA_TCH_FULL && cls != TETRA_TCH_HALF) {
        if (l < NT) o[l] = l == TETRA_TQ_CLASS ? cls : 0;
        return;
    }

    // ---- export: output dword d holds tch bits 4 d .. 4 d + 3 (216, where FULL's second field begins,
    // is a multiple of 4: no dword spans the gap)
    const int n = cls == TETRA_TCH_FULL ? TETRA_TCH_BITS : TETRA_TCH_BITS / 2;
    const uint32_t init = cell_init[ch / G];
    int8_t *out = tch + cb * TETRA_TCH_BITS;
    uint32_t wsum = 0, nzero = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int d = l + TQ_LANES * u;
        if (4 * d < n) {
            const int i = 4 * d;
            const int at = cls == TETRA_TCH_HALF ? 282 + i : i < 216 ? 14 + i : 66 + i;   // 282 + (i - 216)
            const uint32_t sv = load_u32(srow + p0 + at);
            const uint4 mk = *reinterpret_cast<const uint4 *>(&SCR_MASK.w[i]);
            const uint32_t q[4] = {(uint32_t)__popc(init & mk.x) & 1u, (uint32_t)__popc(init & mk.y) & 1u,
                                   (uint32_t)__popc(init & mk.z) & 1u, (uint32_t)__popc(init & mk.w) & 1u};
            uint32_t ov = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int s = (int8_t)(sv >> (8 * k));
                const int t = q[k] ? (s == -128 ? 127 : -s) : s;
                wsum += (uint32_t)(t < 0 ? -t : t);
                nzero += t == 0;
                ov |= ((uint32_t)t & 0xFFu) << (8 * k);
            }
            store_u32(out + i, ov);
        }
    }
    wsum = group_sum(wsum);
    nzero = group_sum(nzero);
    if (l == 0) {
        o[TETRA_TQ_CLASS] = cls;
        o[TETRA_TQ_NBITS] = n;
        o[TETRA_TQ_WSUM] = (int32_t)wsum;
        o[TETRA_TQ_NZERO] = (int32_t)nzero;
    }
}

}  // namespace

extern "C" int tetra_etsi_traffic(tetra_ctx *ctx, const int8_t *softbits, size_t C, size_t stride, int32_t origin_bits,
                                  size_t G, const uint32_t *cell_init, const int32_t *nburst, const int32_t *bursts,
                                  const int32_t *nblock, const int32_t *blocks, const int32_t *slots,
                                  const int32_t *keep, int32_t *tq, int8_t *tch) {
    if (!ctx) return TETRA_E_INVALID;
    if (C == 0 || stride == 0 || !softbits || !cell_init || !nburst || !bursts || !nblock || !blocks || !tq || !tch)
        return tetra_fail(ctx, TETRA_E_INVALID, "tetra_etsi_traffic: C > 0, stride > 0 and every array but slots, keep");
    if (G < 1 || C % G != 0 || origin_bits < 0)
        return tetra_fail(ctx, TETRA_E_INVALID,
                          "tetra_etsi_traffic: G >= 1 rows per cell dividing C and origin_bits >= 0 (C %zu, G %zu, "
                          "origin_bits %d)", C, G, (int)origin_bits);
    if (C > ((size_t)1 << 24) || G > ((size_t)1 << 24) || stride > ((size_t)1 << 28))
        return tetra_fail(ctx, TETRA_E_INVALID, "too many rows or too long a row for one tetra_etsi_traffic call");
    Staging st(ctx);
    // the three small host arrays travel as one staged input (six staged inputs in all)
    Staging::Part small[] = {{cell_init, C / G}, {nburst, C}, {nblock, C}};
    if (!st.pack(small)) return st.finish();
    const uint32_t *ci = (const uint32_t *)small[0].p;
    const int32_t *nb = (const int32_t *)small[1].p, *nk = (const int32_t *)small[2].p;
    const int8_t *sb = (const int8_t *)st.in(softbits, C * stride * 2);
    const int32_t *bu = (const int32_t *)st.in(bursts, C * ETSI_MAXB * 2 * 4);
    const int32_t *bk = (const int32_t *)st.in(blocks, C * ETSI_MAXJ * 4 * 4);
    const int32_t *sl = slots ? (const int32_t *)st.in(slots, C * ETSI_MAXB * TETRA_SLOT_FIELDS * 4) : nullptr;
    const int32_t *kp = keep ? (const int32_t *)st.in(keep, C * ETSI_MAXB * 4) : nullptr;
    // in/out: what the call does not write keeps the caller's contents in host memory too
    int32_t *to = (int32_t *)st.inout(tq, C * ETSI_MAXB * NT * 4);
    int8_t *tc = (int8_t *)st.inout(tch, C * ETSI_MAXB * TETRA_TCH_BITS);
    if (!sb || !bu || !bk || (slots && !sl) || (keep && !kp) || !to || !tc) return st.finish();
    {
        PROF(ctx, "etsi_traffic");
        hipLaunchKernelGGL(k_etsi_traffic, dim3((unsigned)C), dim3(TQ_BLOCK), 0, ctx->stream, sb, (int)C, (long)stride,
                           (int)origin_bits, (int)G, ci, nb, bu, nk, bk, sl, kp, to, tc);
    }
    return st.finish();
}
