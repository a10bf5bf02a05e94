// etsi_llc.hip -- LLC headers, the frame check sequence and TL-SDUs of the ETSI chain's TM-SDUs on gfx950
// (tetra_etsi_llc): the step after etsi_sdu.hip, restated in tests/_etsi_llc_model.py.
//
//   k_llc_whole  k_sdu_walk's layout: 16 lanes per row (4 rows per wave), lane j on block j.  A block with a
//                whole, readable MAC-RESOURCE SDU is loaded as its 40-byte sdu_data row into an LDS bit row;
//                the lane reads the header by funnel reads, runs the CRC-32 a byte a step from a 256-entry
//                table in LDS (built by the workgroup) with the sub-byte tail bitwise, and cuts the TL-SDU.
//   k_llc_done   one wave per group of G rows, as k_sdu_join: ndone == 0 costs one load.  Otherwise a
//                message's bytes go to LDS, and the CRC is split over the lanes from the message's end:
//                lane l runs the eight whole bytes that have 8 l bytes behind them from a zero register,
//                multiplies the partial by x^(64 l) mod P (shift-and-xor, the lane's own constant) and the
//                wave xor-reduces; the 0xFFFFFFFF start is folded into the first 32 bits, the sub-byte tail
//                runs bitwise on the sum.  One __shfl_xor butterfly a message: on this rare path DPP forms
//                would buy nothing that shows.  The TL-SDU is a funnel shift by 4..6 bits, a byte per lane
//                per pass.
#include "common.h"

namespace {

constexpr int MAXJ = TETRA_ETSI_MAXJ, MAXPDU = TETRA_ETSI_MAXPDU, NF = TETRA_PDU_FIELDS, NS = TETRA_SDU_FIELDS;
constexpr int ROWB = TETRA_SDU_ROW, MAXBYTES = TETRA_SDU_MAXBYTES, ND = TETRA_DONE_FIELDS, NL = TETRA_LLC_FIELDS;
constexpr int LLC_LANES = 16;    // lanes per row: one per block
constexpr int LLC_BLOCK = 256;   // 16 rows per workgroup
constexpr int WROW = 11;         // LDS dwords per lane: 40 bytes in 10, one more for the funnel read; odd: no bank conflicts
constexpr int MAXG = 64;
constexpr uint32_t POLY = 0x04C11DB7u;
constexpr int SEG = 8;           // bytes of a message per lane: 64 lanes x 8 = TETRA_SDU_MAXBYTES
static_assert(64 * SEG >= MAXBYTES, "one pass of the wave covers the longest message");
static_assert(ROWB == 4 * (WROW - 1), "an sdu_data row is ten dwords");

// x^(64 l) mod P for lane l: the power that belongs to 8 l bytes behind a segment
struct Pow64 { uint32_t v[64]; };
constexpr Pow64 make_pow64() {
    Pow64 t{};
    uint32_t r = 1;
    for (int l = 0; l < 64; ++l) {
        t.v[l] = r;
        for (int i = 0; i < 64; ++i) r = (r << 1) ^ ((r >> 31) ? POLY : 0u);
    }
    return t;
}
__device__ const Pow64 kPow64 = make_pow64();

// entry i of the byte table: i(x) x^32 mod P
__device__ __forceinline__ uint32_t crc_entry(int i) {
    uint32_t r = (uint32_t)i << 24;
#pragma unroll
    for (int k = 0; k < 8; ++k) r = (r << 1) ^ ((r >> 31) ? POLY : 0u);
    return r;
}
__device__ __forceinline__ uint32_t crc_byte(uint32_t r, uint32_t b, const uint32_t *tab) {
    return (r << 8) ^ tab[(r >> 24) ^ b];
}
__device__ __forceinline__ uint32_t crc_bit(uint32_t r, uint32_t b) {
    const uint32_t t = (r >> 31) ^ b;
    r <<= 1;
    return t ? r ^ POLY : r;
}
// a(x) b(x) mod P, shift and xor
__device__ __forceinline__ uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll 8
    for (int i = 31; i >= 0; --i) {
        r = (r << 1) ^ ((r >> 31) ? POLY : 0u);
        if ((b >> i) & 1) r ^= a;
    }
    return r;
}

// n in 1..32 bits from bit `off` of an MSB-first bit row (bit p is bit 31 - (p & 31) of dword p >> 5)
__device__ __forceinline__ uint32_t field(const uint32_t *w, int off, int n) {
    const int q = off >> 5, s = off & 31;
    const uint64_t v = ((uint64_t)w[q] << 32) | w[q + 1];
    const uint32_t x = (uint32_t)(v >> (64 - s - n));
    return n == 32 ? x : x & ((1u << n) - 1);
}

// What the first four bits decide: header bits, the sequence bits, whether an FCS closes the PDU.
struct Header {
    int status, type, nr, ns, off, nbits, fcs;   // nbits: the TL-SDU's
};
// n: the PDU's bits; first6: its first min(n, 6) bits, left-aligned in 6
__device__ __forceinline__ Header parse(int n, uint32_t first6) {
    Header h{TETRA_LLC_MALFORMED, 0, -1, -1, 0, 0, 0};
    if (n < 4) return h;
    const int type = (int)(first6 >> 2);
    if (type >= 8) {
        h.status = TETRA_LLC_UNSUPPORTED;
        h.type = type;
        return h;
    }
    const int form = type & 3;   // 0 BL-ADATA, 1 BL-DATA, 2 BL-UDATA, 3 BL-ACK
    const int hdr = form == 0 ? 6 : form == 2 ? 4 : 5;
    const int need = hdr + ((type & 4) ? 32 : 0);
    if (n < need) return h;
    h.status = TETRA_LLC_OK;
    h.type = type;
    if (form == 0) h.nr = (first6 >> 1) & 1, h.ns = first6 & 1;
    if (form == 1) h.ns = (first6 >> 1) & 1;
    if (form == 3) h.nr = (first6 >> 1) & 1;
    h.off = hdr;
    h.nbits = n - need;
    h.fcs = (type & 4) ? 1 : 0;
    return h;
}

__device__ __forceinline__ void put(int32_t *o, const Header &h, int head, uint32_t rx, uint32_t calc) {
    o[TETRA_LLC_STATUS] = h.status;
    o[TETRA_LLC_TYPE] = h.type;
    o[TETRA_LLC_NR] = h.nr;
    o[TETRA_LLC_NS] = h.ns;
    o[TETRA_LLC_OFFSET] = h.off;
    o[TETRA_LLC_NBITS] = h.nbits;
    o[TETRA_LLC_HEAD] = head;
    o[TETRA_LLC_FCS] = h.fcs == 0 ? TETRA_FCS_NONE : rx == calc ? TETRA_FCS_GOOD : TETRA_FCS_BAD;
    o[TETRA_LLC_FCS_RX] = (int32_t)rx;
    o[TETRA_LLC_FCS_CALC] = (int32_t)calc;
}

// Grid: 16 lanes per row, LLC_BLOCK / 16 rows per workgroup; the lanes past C idle.
__global__ __launch_bounds__(LLC_BLOCK) void k_llc_whole(int C, const int32_t *__restrict__ nblock,
                                                         const int32_t *__restrict__ blocks,
                                                         const int32_t *__restrict__ npdu,
                                                         const int32_t *__restrict__ pdus,
                                                         const int32_t *__restrict__ sdu,
                                                         const uint8_t *__restrict__ sdu_data,
                                                         int32_t *__restrict__ llc, uint8_t *__restrict__ tl) {
    __shared__ uint32_t rows[LLC_BLOCK * WROW];
    __shared__ uint32_t tab[256];
    const int tid = threadIdx.x, j = tid & (LLC_LANES - 1);
    const long ch = (long)blockIdx.x * (LLC_BLOCK / LLC_LANES) + tid / LLC_LANES;
    tab[tid] = crc_entry(tid);
    __syncthreads();
    if (ch >= C || j >= min(max(nblock[ch], 0), MAXJ)) return;
    const size_t cj = (size_t)ch * MAXJ + j;
    const int kind = blocks[4 * cj], crc = blocks[4 * cj + 1];
    const int n = crc != 0 && kind >= TETRA_SCH_F && kind <= TETRA_BSCH ? min(max(npdu[cj], 0), MAXPDU) : 0;
    if (n == 0) return;
    // what each record is, before the row is touched: most blocks carry no LLC PDU
    int what[MAXPDU];
    bool any = false;
#pragma unroll
    for (int q = 0; q < MAXPDU; ++q) {
        what[q] = TETRA_LLC_NONE;
        if (q < n) {
            const int32_t *p = pdus + (cj * MAXPDU + q) * NF, *s = sdu + (cj * MAXPDU + q) * NS;
            const int st = s[TETRA_SDU_STATUS], sn = s[TETRA_SDU_NBITS], at = s[TETRA_SDU_BYTE];
            if (p[TETRA_PDU_KIND] == TETRA_PDU_RESOURCE && s[TETRA_SDU_ROLE] == TETRA_ROLE_WHOLE) {
                if (st == TETRA_SDU_ENCRYPTED || p[TETRA_PDU_ENC] != 0) what[q] = TETRA_LLC_ENCRYPTED;
                else if (st == TETRA_SDU_OK && sn > 0)   // an extent outside the row: nothing is read
                    what[q] = at >= 0 && sn <= 8 * ROWB && at + ((sn + 7) >> 3) <= ROWB ? TETRA_LLC_OK : TETRA_LLC_MALFORMED;
            }
            any |= what[q] == TETRA_LLC_OK;
        }
    }
    uint32_t *w = rows + tid * WROW;
    if (any) {
        const uint8_t *t = sdu_data + cj * ROWB;
        if (((uintptr_t)sdu_data & 3) == 0) {
#pragma unroll
            for (int i = 0; i < WROW - 1; ++i) w[i] = __builtin_bswap32(reinterpret_cast<const uint32_t *>(t)[i]);
        } else {
            for (int i = 0; i < WROW - 1; ++i)
                w[i] = (uint32_t)t[4 * i] << 24 | (uint32_t)t[4 * i + 1] << 16 | (uint32_t)t[4 * i + 2] << 8 | t[4 * i + 3];
        }
        w[WROW - 1] = 0;
    }
#pragma unroll
    for (int q = 0; q < MAXPDU; ++q) {
        if (q >= n) break;
        int32_t *o = llc + (cj * MAXPDU + q) * NL;
        Header h{what[q], what[q] == TETRA_LLC_ENCRYPTED ? -1 : 0, -1, -1, 0, 0, 0};
        int head = 0;
        uint32_t rx = 0, calc = 0;
        if (what[q] == TETRA_LLC_OK) {
            const int32_t *s = sdu + (cj * MAXPDU + q) * NS;
            const int sn = s[TETRA_SDU_NBITS], at = s[TETRA_SDU_BYTE], base = 8 * at;
            const int n6 = min(sn, 6);
            h = parse(sn, field(w, base, n6) << (6 - n6));
            if (h.status == TETRA_LLC_OK) {
                if (h.fcs) {
                    const int L = sn - 32, nfull = L >> 3;
                    uint32_t r = 0xFFFFFFFFu;
                    for (int i = 0; i < nfull; ++i) r = crc_byte(r, field(w, base + 8 * i, 8), tab);
                    for (int i = 8 * nfull; i < L; ++i) r = crc_bit(r, field(w, base + i, 1));
                    calc = ~r;
                    rx = field(w, base + L, 32);
                }
                const int nh = min(h.nbits, 8);
                head = h.nbits < 3 ? -1 : (int)(field(w, base + h.off, nh) << (8 - nh));
                uint8_t *dst = tl + cj * ROWB + at;
                const int nby = (h.nbits + 7) >> 3;
                for (int i = 0; i < nby; ++i) {
                    const int nb = min(8, h.nbits - 8 * i);
                    dst[i] = (uint8_t)(field(w, base + h.off + 8 * i, nb) << (8 - nb));
                }
            }
        }
        put(o, h, head, rx, calc);
    }
}

// One wave per group.  The workgroup must stay one wave of 64: the xor butterfly spans it.
__global__ __launch_bounds__(64) void k_llc_done(int maxd, const int32_t *__restrict__ ndone,
                                                 const int32_t *__restrict__ done,
                                                 const uint8_t *__restrict__ done_data,
                                                 int32_t *__restrict__ llc_done, uint8_t *__restrict__ tl_done) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t msgw[MAXBYTES / 4 + 2];
    uint8_t *msg = reinterpret_cast<uint8_t *>(msgw);
    const int lane = threadIdx.x;
    const size_t g = blockIdx.x;
    const int nd = min(max(ndone[g], 0), maxd);
    if (nd == 0) return;   // nearly every group of a step
#pragma unroll
    for (int i = 0; i < 4; ++i) tab[4 * lane + i] = crc_entry(4 * lane + i);
    const uint32_t pw = kPow64.v[lane];
    for (int m = 0; m < nd; ++m) {
        const size_t di = g * (size_t)maxd + m;
        const int32_t *rec = done + di * ND;
        const int enc = rec[TETRA_DONE_ENC], sn = rec[TETRA_DONE_NBITS];
        int32_t *o = llc_done + di * NL;
        Header h{TETRA_LLC_NONE, 0, -1, -1, 0, 0, 0};
        if (enc != 0) h.status = TETRA_LLC_ENCRYPTED, h.type = -1;
        else if (sn < 0 || sn > 8 * MAXBYTES) h.status = TETRA_LLC_MALFORMED;   // no record of tetra_etsi_sdu's
        else if (sn > 0) h.status = TETRA_LLC_OK;
        if (h.status != TETRA_LLC_OK) {
            if (lane == 0) put(o, h, 0, 0, 0);
            continue;
        }
        const uint8_t *src = done_data + di * MAXBYTES;
        const int nsrc = (sn + 7) >> 3;
        __syncthreads();   // the previous message's readers are through
        if (((uintptr_t)done_data & 3) == 0) {
            for (int i = lane; i < (nsrc + 3) >> 2; i += 64)
                msgw[i] = reinterpret_cast<const uint32_t *>(src)[i];
        } else {
            for (int i = lane; i < nsrc; i += 64) msg[i] = src[i];
        }
        __syncthreads();
        const int n6 = min(sn, 6);
        h = parse(sn, ((uint32_t)(msg[0] >> 2) >> (6 - n6)) << (6 - n6));
        if (h.status != TETRA_LLC_OK) {
            if (lane == 0) put(o, h, 0, 0, 0);
            continue;
        }
        uint32_t rx = 0, calc = 0;
        if (h.fcs) {
            const int L = sn - 32, nfull = L >> 3, tb = L & 7;
            // lane l: the whole bytes [nfull - 8 (l + 1), nfull - 8 l), from a zero register; the start
            // value is the first 32 bits inverted
            uint32_t r = 0;
            const int hi = nfull - SEG * lane, lo = max(hi - SEG, 0);
            for (int i = lo; i < hi; ++i) r = crc_byte(r, msg[i] ^ (i < 4 ? 0xFFu : 0u), tab);
            r = hi > 0 ? mulmod(r, pw) : 0u;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) r ^= (uint32_t)__shfl_xor((int)r, d);
            for (int t = 0; t < tb; ++t) {
                const int p = 8 * nfull + t;
                r = crc_bit(r, ((msg[nfull] >> (7 - t)) & 1u) ^ (p < 32 ? 1u : 0u));
            }
            if (L < 32) r ^= 0xFFFFFFFFu << L;   // the part of the start value the message does not reach
            calc = ~r;
            uint64_t v = 0;   // the 32 bits at bit L
            for (int i = 0; i < 5; ++i) v = v << 8 | (nfull + i < nsrc ? msg[nfull + i] : 0u);
            rx = (uint32_t)(v >> (8 - tb));
        }
        const int nby = (h.nbits + 7) >> 3;
        for (int t = lane; t < nby; t += 64) {   // byte t of the TL-SDU from bytes t and t + 1 of the message
            const int nb = min(8, h.nbits - 8 * t);
            const uint32_t two = (uint32_t)msg[t] << 8 | (t + 1 < nsrc ? msg[t + 1] : 0u);
            tl_done[di * MAXBYTES + t] = (uint8_t)((two >> (8 - h.off)) & (0xFFu << (8 - nb)) & 0xFFu);
        }
        if (lane == 0) {
            const int nh = min(h.nbits, 8);
            const uint32_t two = (uint32_t)msg[0] << 8 | (nsrc > 1 ? msg[1] : 0u);
            const int head = h.nbits < 3 ? -1 : (int)((two >> (8 - h.off)) & (0xFFu << (8 - nh)) & 0xFFu);
            put(o, h, head, rx, calc);
        }
    }
}

}  // namespace

extern "C" int tetra_etsi_llc(tetra_ctx *ctx, size_t C, size_t G, const int32_t *nblock, const int32_t *blocks,
                              const int32_t *npdu, const int32_t *pdus, const int32_t *sdu, const uint8_t *sdu_data,
                              int32_t maxd, const int32_t *ndone, const int32_t *done, const uint8_t *done_data,
                              int32_t *llc, uint8_t *tl, int32_t *llc_done, uint8_t *tl_done) {
    if (!ctx) return TETRA_E_INVALID;
    if (C == 0 || !nblock || !blocks || !npdu || !pdus || !sdu || !sdu_data || !ndone || !llc || !tl ||
        (maxd > 0 && (!done || !done_data || !llc_done || !tl_done)))
        return tetra_fail(ctx, TETRA_E_INVALID, "tetra_etsi_llc: C > 0 and every array (the four done arrays when maxd > 0)");
    if (G < 1 || G > (size_t)MAXG || C % G != 0 || maxd < 0)
        return tetra_fail(ctx, TETRA_E_INVALID,
                          "tetra_etsi_llc: 1 <= G <= %d rows per group dividing C, maxd >= 0 (C %zu, G %zu, maxd %d)", MAXG,
                          C, G, (int)maxd);
    if (C > ((size_t)1 << 24)) return tetra_fail(ctx, TETRA_E_INVALID, "too many rows for one tetra_etsi_llc call (%zu)", C);
    const size_t NG = C / G;
    Staging st(ctx);
    // the int32 host inputs but the PDU and SDU records travel as one staged input (five staged inputs in all)
    Staging::Part small[] = {{nblock, C}, {npdu, C * MAXJ}, {ndone, NG}, {blocks, C * MAXJ * 4},
                             {maxd > 0 ? done : nullptr, NG * (size_t)maxd * ND}};
    if (!st.pack(small)) return st.finish();
    const int32_t *nk = (const int32_t *)small[0].p, *np = (const int32_t *)small[1].p, *nd = (const int32_t *)small[2].p,
                  *bk = (const int32_t *)small[3].p, *dn = (const int32_t *)small[4].p;
    const int32_t *pd = (const int32_t *)st.in(pdus, C * MAXJ * MAXPDU * NF * 4);
    const int32_t *sr = (const int32_t *)st.in(sdu, C * MAXJ * MAXPDU * NS * 4);
    const uint8_t *sd = (const uint8_t *)st.in(sdu_data, C * MAXJ * ROWB);
    const uint8_t *dd = maxd > 0 ? (const uint8_t *)st.in(done_data, NG * (size_t)maxd * MAXBYTES) : nullptr;
    // in/out: what the kernels do not write keeps the caller's contents in host memory too
    int32_t *lo = (int32_t *)st.inout(llc, C * MAXJ * MAXPDU * NL * 4);
    uint8_t *to = (uint8_t *)st.inout(tl, C * MAXJ * ROWB);
    int32_t *ld = maxd > 0 ? (int32_t *)st.inout(llc_done, NG * (size_t)maxd * NL * 4) : nullptr;
    uint8_t *td = maxd > 0 ? (uint8_t *)st.inout(tl_done, NG * (size_t)maxd * MAXBYTES) : nullptr;
    if (!pd || !sr || !sd || !lo || !to || (maxd > 0 && (!dd || !ld || !td))) return st.finish();
    {
        PROF(ctx, "etsi_llc");
        hipLaunchKernelGGL(k_llc_whole, dim3(grid_for(C * LLC_LANES, LLC_BLOCK)), dim3(LLC_BLOCK), 0, ctx->stream, (int)C,
                           nk, bk, np, pd, sr, sd, lo, to);
        if (maxd > 0)
            hipLaunchKernelGGL(k_llc_done, dim3((unsigned)NG), dim3(64), 0, ctx->stream, (int)maxd, nd, dn, dd, ld, td);
    }
    return st.finish();
}
