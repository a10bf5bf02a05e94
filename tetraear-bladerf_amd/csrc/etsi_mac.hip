// etsi_mac.hip -- TDMA timebase and MAC PDU headers of the ETSI chain's decoded blocks on gfx950
// (tetra_etsi_mac): the step after etsi_lmac.hip, restated in tests/_etsi_mac_model.py.
//
//   k_etsi_mac  16 lanes per channel (4 channels per wave), lane j on block j: a CRC-good block's
//               type-1 bytes are packed into an LDS bit row (dword loads, four bits per multiply),
//               the lane walks its PDUs from that row and writes their records; the group's first
//               lane then runs the channel's timebase over its bursts, taking a synchronisation
//               burst's slot count from the lane that parsed its BSCH block (through LDS).
//   k_mac_walk, k_tdma_groups  (tetra_etsi_mac_groups, restated in tests/_etsi_mac_groups.py): the same
//               block walk, then per group of overlapping rows -- a wideband carrier's chunks -- one
//               wave that rank-sorts the group's bursts by position in LDS, keeps each burst once and
//               runs one timebase over the merged order.
#include "etsi_mac.h"

namespace {

constexpr int MAXB = TETRA_ETSI_MAXB, MAXJ = TETRA_ETSI_MAXJ, MAXPDU = TETRA_ETSI_MAXPDU, NF = TETRA_PDU_FIELDS;
constexpr int MAC_LANES = 16;    // lanes per channel: one per block
constexpr int MAC_BLOCK = 256;   // 16 channels per workgroup
constexpr int WROW = 11;         // LDS dwords per lane: 268 bits in 9, one more for the funnel read; odd: no bank conflicts

// n <= 24 bits from bit `off` of an MSB-first bit row (bit p is bit 31 - (p & 31) of dword p >> 5)
__device__ __forceinline__ int field(const uint32_t *w, int off, int n) {
    const int q = off >> 5, s = off & 31;
    const uint64_t v = ((uint64_t)w[q] << 32) | w[q + 1];
    return (int)((uint32_t)(v >> (64 - s - n)) & ((1u << n) - 1));
}

// The first n1 bytes of a block (a multiple of 4) as bits, four per dword load: (v & 0x01010101) *
// 0x08040201 gathers bytes 0..3 into bits 27..24 with no carries.  The dwords past n1 read 0.
__device__ __forceinline__ void pack_block(const uint8_t *t, int n1, bool al4, uint32_t *w) {
    const int nd = n1 >> 2;
    for (int wi = 0; wi < WROW; ++wi) {
        uint32_t acc = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = 8 * wi + u;
            uint32_t v = 0;
            if (i < nd) {
                if (al4) v = reinterpret_cast<const uint32_t *>(t)[i];
                else v = t[4 * i] | (uint32_t)t[4 * i + 1] << 8 | (uint32_t)t[4 * i + 2] << 16 | (uint32_t)t[4 * i + 3] << 24;
            }
            acc = (acc << 4) | (((v & 0x01010101u) * 0x08040201u) >> 24);
        }
        w[wi] = acc;
    }
}

struct Rec {
    int32_t f[NF];
};

__device__ __forceinline__ void put_rec(int32_t *p, const Rec &r) {
#pragma unroll
    for (int i = 0; i < NF; ++i) p[i] = r.f[i];
}

// Length indication (pi/4-DQPSK): the PDU's bits with `rem` bits left in the block; 1 = malformed.
__device__ __forceinline__ int pdu_length(int L, int rem, int &nbits) {
    nbits = rem;
    if (L >= 2 && L <= 34) {
        if (8 * L <= rem) nbits = 8 * L;
        else if (8 * L - rem >= 8) return 1;
        return 0;
    }
    return L == 62 || L == 63 ? 0 : 1;
}

// SYNC PDU of a BSCH block; returns the slot count, -1 when FN or MN is out of range.
__device__ __forceinline__ int parse_sync(const uint32_t *w, Rec &r) {
    const int tn = field(w, 10, 2), fn = field(w, 12, 5), mn = field(w, 17, 6);
    const bool ok = fn >= 1 && fn <= 18 && mn >= 1 && mn <= 60;
    r.f[TETRA_PDU_KIND] = TETRA_PDU_SYNC;
    r.f[TETRA_PDU_OFFSET] = 0;
    r.f[TETRA_PDU_NBITS] = 60;
    r.f[TETRA_PDU_STATUS] = !ok;
    r.f[4] = field(w, 0, 4);
    r.f[5] = field(w, 4, 6);
    r.f[6] = tn;
    r.f[7] = fn;
    r.f[8] = mn;
    r.f[9] = field(w, 23, 2);
    r.f[10] = field(w, 25, 3);
    r.f[11] = field(w, 28, 1) | field(w, 29, 1) << 1 | field(w, 59, 1) << 2;
    r.f[12] = field(w, 31, 10);
    r.f[13] = field(w, 41, 14);
    r.f[14] = field(w, 55, 2);
    r.f[15] = field(w, 57, 2);
    return ok ? ((mn - 1) * 18 + (fn - 1)) * 4 + tn : -1;
}

// One downlink MAC PDU at bit `off` of an SCH block of n1 bits (n1 - off >= 16); returns the bits to
// advance by, 0 when the walk stops here.
__device__ __forceinline__ int parse_pdu(const uint32_t *w, int off, int n1, Rec &r) {
    const int rem = n1 - off;
#pragma unroll
    for (int i = 0; i < NF; ++i) r.f[i] = 0;
    r.f[TETRA_PDU_OFFSET] = off;
    r.f[TETRA_PDU_NBITS] = rem;
    const int t = field(w, off, 2);
    if (t == 0) {   // MAC-RESOURCE
        const int L = field(w, off + 7, 6), at = field(w, off + 13, 3);
        r.f[TETRA_PDU_FILL] = field(w, off + 2, 1);
        r.f[TETRA_PDU_ENC] = field(w, off + 4, 2);
        r.f[TETRA_PDU_LENGTH] = L;
        r.f[TETRA_PDU_ADDR_TYPE] = at;
        r.f[TETRA_PDU_SSI] = -1;
        r.f[TETRA_PDU_AUX] = -1;
        r.f[TETRA_PDU_FLAGS] = field(w, off + 3, 1) | field(w, off + 6, 1) << 1;
        if (at == 0) {   // null PDU: 16 bits, nothing follows
            r.f[TETRA_PDU_KIND] = TETRA_PDU_NULL;
            r.f[TETRA_PDU_NBITS] = 16;
            r.f[TETRA_PDU_HDR_BITS] = 16;
            return 0;
        }
        r.f[TETRA_PDU_KIND] = TETRA_PDU_RESOURCE;
        int nbits;
        int status = pdu_length(L, rem, nbits);
        const bool ssi = at != 2, aux = at == 2 || at >= 5;
        const int auxn = at == 6 ? 6 : 10;
        const int hdr = 16 + (ssi ? 24 : 0) + (aux ? auxn : 0);
        if (hdr > nbits) {
            status = 1;   // the address runs past the PDU (or block) end: not read
        } else {
            if (ssi) r.f[TETRA_PDU_SSI] = field(w, off + 16, 24);
            if (aux) r.f[TETRA_PDU_AUX] = field(w, off + 16 + (ssi ? 24 : 0), auxn);
        }
        r.f[TETRA_PDU_NBITS] = nbits;
        r.f[TETRA_PDU_STATUS] = status;
        r.f[TETRA_PDU_HDR_BITS] = hdr;
        return status == 0 && L <= 34 ? 8 * L : 0;
    }
    if (t == 1) {
        r.f[TETRA_PDU_SSI] = -1;
        r.f[TETRA_PDU_AUX] = -1;
        r.f[TETRA_PDU_FILL] = field(w, off + 3, 1);
        if (field(w, off + 2, 1) == 0) {   // MAC-FRAG: the rest of the block
            r.f[TETRA_PDU_KIND] = TETRA_PDU_FRAG;
            r.f[TETRA_PDU_HDR_BITS] = 4;
            return 0;
        }
        const int L = field(w, off + 5, 6);   // MAC-END
        int nbits;
        const int status = pdu_length(L, rem, nbits);
        r.f[TETRA_PDU_KIND] = TETRA_PDU_END;
        r.f[TETRA_PDU_NBITS] = nbits;
        r.f[TETRA_PDU_STATUS] = status;
        r.f[TETRA_PDU_LENGTH] = L;
        r.f[TETRA_PDU_HDR_BITS] = 11;
        r.f[TETRA_PDU_FLAGS] = field(w, off + 4, 1);
        return status == 0 && L <= 34 ? 8 * L : 0;
    }
    if (t == 3) {
        r.f[TETRA_PDU_KIND] = TETRA_PDU_SUPPL;
        return 0;
    }
    const int sub = field(w, off + 2, 2);   // broadcast
    r.f[TETRA_PDU_KIND] = sub == 0 ? TETRA_PDU_SYSINFO : sub == 1 ? TETRA_PDU_ACCESS_DEFINE : TETRA_PDU_BROADCAST;
    if (sub != 0) return 0;
    if (rem < 124) {
        r.f[TETRA_PDU_STATUS] = 1;
        return 0;
    }
    r.f[TETRA_PDU_NBITS] = 124;
    r.f[4] = field(w, off + 4, 12);
    r.f[5] = field(w, off + 16, 4);
    r.f[6] = field(w, off + 20, 2);
    r.f[7] = field(w, off + 22, 3);
    r.f[8] = field(w, off + 25, 1);
    r.f[9] = field(w, off + 26, 2);
    r.f[10] = field(w, off + 28, 3);
    r.f[11] = field(w, off + 31, 4);
    r.f[12] = field(w, off + 35, 4) | field(w, off + 39, 4) << 4 | field(w, off + 60, 2) << 8;
    r.f[13] = field(w, off + 43, 1) << 16 | field(w, off + 44, 16);
    r.f[14] = field(w, off + 82, 14);
    r.f[15] = field(w, off + 96, 16) | field(w, off + 112, 12) << 16;
    return 0;
}

// The channel's timebase over its bursts (one lane): sync_slot[q] is the slot count of the STATUS 0
// SYNC record of the channel's block q, -1 where block q gave none.
__device__ __forceinline__ void timebase(int nb, const int32_t *__restrict__ bursts, const int *sync_slot, int nsym,
                                         tetra_etsi_tdma *td, int32_t *__restrict__ slots) {
    int64_t bit0 = td->bit0, abit = td->anchor_bit;
    int aslot = td->anchor_slot;
    bool locked = td->locked != 0;
    int q = 0;   // block of burst b: the sync kernel's numbering (1 per NDB(n), 2 per NDB(p) / SB)
    for (int b = 0; b < nb; ++b) {
        const int64_t p = bit0 + bursts[2 * b];
        const int kind = bursts[2 * b + 1];
        const bool was = locked;
        int pred = -1;   // rule 2: the slot the grid gives this burst
        if (locked) {
            const int64_t d = p - abit;
            const int64_t k = d >= 0 ? (d + 255) / 510 : TETRA_TDMA_EXPIRE;
            if (k >= TETRA_TDMA_EXPIRE) {
                locked = false;
            } else {
                const int64_t r = d - 510 * k;
                if (r >= -TETRA_TDMA_TOL && r <= TETRA_TDMA_TOL) pred = (int)((aslot + k) % TETRA_TDMA_SLOTS);
            }
        }
        const int own = kind == TETRA_SB && q < MAXJ ? sync_slot[q] : -1;   // rule 1: the burst's own SYNC
        int slot = pred, flags = 0;
        if (own >= 0) {
            slot = own;
            flags = 1 | (was && pred != own ? 2 : 0);
            locked = true;
        }
        if (slot >= 0) {
            abit = p;
            aslot = slot;
        }
        int32_t *row = slots + TETRA_SLOT_FIELDS * b;
        row[TETRA_SLOT_TN] = slot >= 0 ? slot % 4 + 1 : 0;
        row[TETRA_SLOT_FN] = slot >= 0 ? slot / 4 % 18 + 1 : 0;
        row[TETRA_SLOT_MN] = slot >= 0 ? slot / 72 + 1 : 0;
        row[TETRA_SLOT_FLAGS] = flags;
        q += kind == TETRA_NDB_N ? 1 : 2;
    }
    td->bit0 = bit0 + 2 * (int64_t)max(nsym - 1, 0);
    td->anchor_bit = abit;
    td->anchor_slot = aslot;
    td->locked = locked;
}

// Lane j of channel ch walks its block j into rows + tid * WROW and writes npdu / pdus; returns the
// slot count of the block's STATUS 0 SYNC record, -1 where it gave none.  Shared by both kernels.
__device__ __forceinline__ int walk_block(bool act, long ch, int j, int tid, uint32_t *rows,
                                          const int32_t *__restrict__ nblock, const int32_t *__restrict__ blocks,
                                          const uint8_t *__restrict__ type1, int32_t *__restrict__ npdu,
                                          int32_t *__restrict__ pdus) {
    int own = -1;
    if (act) {
        const size_t cj = (size_t)ch * MAXJ + j;
        const int nk = min(max(nblock[ch], 0), MAXJ);
        int count = 0;
        if (j < nk) {
            const int kind = blocks[4 * cj], crc = blocks[4 * cj + 1];
            if (crc != 0 && kind >= TETRA_SCH_F && kind <= TETRA_BSCH) {
                const int n1 = kind == TETRA_SCH_F ? 268 : kind == TETRA_SCH_HD ? 124 : 60;
                uint32_t *w = rows + tid * WROW;
                pack_block(type1 + cj * 268, n1, ((uintptr_t)type1 & 3) == 0, w);
                int32_t *out = pdus + cj * MAXPDU * NF;
                Rec r;
                if (kind == TETRA_BSCH) {
                    own = parse_sync(w, r);
                    put_rec(out, r);
                    count = 1;
                } else {
                    for (int off = 0; n1 - off >= 16;) {
                        const int adv = parse_pdu(w, off, n1, r);
                        if (count < MAXPDU) put_rec(out + count * NF, r);
                        ++count;
                        if (adv == 0) break;
                        off += adv;
                    }
                }
            }
        }
        npdu[cj] = count;
    }
    return own;
}

// Grid: 16 lanes per channel, MAC_BLOCK / 16 channels per workgroup; the lanes past C idle.
__global__ __launch_bounds__(MAC_BLOCK) void k_etsi_mac(int C, const int32_t *__restrict__ nsym,
                                                        const int32_t *__restrict__ nburst,
                                                        const int32_t *__restrict__ bursts,
                                                        const int32_t *__restrict__ nblock,
                                                        const int32_t *__restrict__ blocks,
                                                        const uint8_t *__restrict__ type1, tetra_etsi_tdma *tdma,
                                                        int32_t *__restrict__ slots, int32_t *__restrict__ npdu,
                                                        int32_t *__restrict__ pdus) {
    __shared__ uint32_t rows[MAC_BLOCK * WROW];
    __shared__ int sync_slot[MAC_BLOCK];
    const int tid = threadIdx.x, j = tid & (MAC_LANES - 1);
    const long ch = (long)blockIdx.x * (MAC_BLOCK / MAC_LANES) + tid / MAC_LANES;
    const bool act = ch < C;
    sync_slot[tid] = walk_block(act, ch, j, tid, rows, nblock, blocks, type1, npdu, pdus);
    __syncthreads();
    if (act && j == 0)
        timebase(min(max(nburst[ch], 0), MAXB), bursts + (size_t)ch * MAXB * 2, sync_slot + tid, nsym[ch], tdma + ch,
                 slots + (size_t)ch * MAXB * TETRA_SLOT_FIELDS);
}

// ---------------------------------------------------------------- groups of overlapping rows
// tetra_etsi_mac_groups: k_etsi_mac's block walk (k_mac_walk: the same lanes, no timebase; lane b < 8
// of a row leaves burst b's own-SYNC slot count, -1 for none, in own [C][MAXB]), then k_tdma_groups,
// one wave per group of G rows: merge_chunks and the timebase over the group's bursts in the order
// (pos, row, b), pos = row * row_bits + start bit.
constexpr int MAXG = 64, MAXE = MAXG * MAXB;   // rows per group, burst entries per group
constexpr int64_t K_SPAN = 510 * (int64_t)TETRA_TDMA_EXPIRE - 255;   // d >= K_SPAN: k >= EXPIRE; d < -K_SPAN: k <= -EXPIRE

__global__ __launch_bounds__(MAC_BLOCK) void k_mac_walk(int C, const int32_t *__restrict__ nburst,
                                                        const int32_t *__restrict__ bursts,
                                                        const int32_t *__restrict__ nblock,
                                                        const int32_t *__restrict__ blocks,
                                                        const uint8_t *__restrict__ type1, int32_t *__restrict__ own,
                                                        int32_t *__restrict__ npdu, int32_t *__restrict__ pdus) {
    __shared__ uint32_t rows[MAC_BLOCK * WROW];
    __shared__ int sync_slot[MAC_BLOCK];
    const int tid = threadIdx.x, j = tid & (MAC_LANES - 1);
    const long ch = (long)blockIdx.x * (MAC_BLOCK / MAC_LANES) + tid / MAC_LANES;
    const bool act = ch < C;
    sync_slot[tid] = walk_block(act, ch, j, tid, rows, nblock, blocks, type1, npdu, pdus);
    __syncthreads();
    if (act && j < min(max(nburst[ch], 0), MAXB)) {   // lane b: the block of burst b by the sync kernel's numbering
        const int32_t *bu = bursts + (size_t)ch * MAXB * 2;
        int q = 0;
        for (int b = 0; b < j; ++b) q += bu[2 * b + 1] == TETRA_NDB_N ? 1 : 2;
        own[(size_t)ch * MAXB + j] = bu[2 * j + 1] == TETRA_SB && q < MAXJ ? sync_slot[tid - j + q] : -1;
    }
}

// One wave per group.  Entry e = row * MAXB + b, so the order (pos, row, b) is (pos, e).
__global__ __launch_bounds__(64) void k_tdma_groups(int G, int64_t row_bits, int64_t tol_bits, int64_t advance,
                                                    const int32_t *__restrict__ nburst,
                                                    const int32_t *__restrict__ bursts,
                                                    const int32_t *__restrict__ own, tetra_etsi_tdma *tdma,
                                                    int32_t *__restrict__ keep, int32_t *__restrict__ slots) {
    __shared__ int64_t pos[MAXE];
    __shared__ int32_t ownv[MAXE];    // own-SYNC slot count, -1 none, DEAD past the row's nburst
    __shared__ int32_t res[MAXE];     // by entry: slot | flags << 16, -1 unknown
    __shared__ uint16_t order[MAXE];  // rank -> entry
    __shared__ int nlive;
    constexpr int32_t DEAD = INT32_MIN;
    const int lane = threadIdx.x, ne = G * MAXB;
    const size_t c0 = (size_t)blockIdx.x * G;
    if (lane == 0) nlive = 0;
    __syncthreads();
    int mine = 0;
    for (int e = lane; e < ne; e += 64) {
        const int i = e / MAXB, b = e % MAXB;
        const bool live = b < min(max(nburst[c0 + i], 0), MAXB);
        pos[e] = live ? (int64_t)((uint64_t)i * (uint64_t)row_bits) + bursts[((c0 + i) * MAXB + b) * 2] : 0;
        ownv[e] = live ? own[(c0 + i) * MAXB + b] : DEAD;
        mine += live;
    }
    if (mine) atomicAdd(&nlive, mine);
    __syncthreads();
    for (int e = lane; e < ne; e += 64) {   // rank sort: exact and stable
        if (ownv[e] == DEAD) continue;
        const int64_t pe = pos[e];
        int rank = 0;
#pragma unroll 8
        for (int f = 0; f < ne; ++f) {   // ne is a multiple of 8: eight LDS read pairs in flight
            const int64_t pf = pos[f];
            rank += (int)(ownv[f] != DEAD) & ((int)(pf < pe) | ((int)(pf == pe) & (int)(f < e)));   // no branches
        }
        order[rank] = (uint16_t)e;
    }
    __syncthreads();
    const int n = nlive;
    for (int r = lane; r < n; r += 64) {   // merge_chunks' chain rule: against the previous in order
        const int e = order[r];
        keep[(c0 + e / MAXB) * MAXB + e % MAXB] = r == 0 || pos[e] - pos[order[r - 1]] > tol_bits;
    }
    if (lane == 0) {
        tetra_etsi_tdma *td = tdma + blockIdx.x;
        const int64_t bit0 = td->bit0;
        int64_t abit = td->anchor_bit;
        int aslot = td->anchor_slot;
        bool locked = td->locked != 0;
        for (int r = 0; r < n; ++r) {
            const int e = order[r];
            const int64_t p = bit0 + pos[e];
            const bool was = locked;
            int pred = -1, k = 0;
            if (locked) {
                const int64_t d = p - abit;
                if (d >= K_SPAN) {
                    locked = false;
                } else if (d >= -K_SPAN) {
                    const int x = (int)d + 255;
                    k = x >= 0 ? x / 510 : -((509 - x) / 510);
                    const int rr = (int)d - 510 * k;
                    if (rr >= -TETRA_TDMA_TOL && rr <= TETRA_TDMA_TOL)
                        pred = (aslot + k + TETRA_TDMA_SLOTS) % TETRA_TDMA_SLOTS;
                }
            }
            const int mine_slot = ownv[e];
            int out = pred;
            if (mine_slot >= 0) {
                out = mine_slot | (1 | (was && pred != mine_slot ? 2 : 0)) << 16;
                abit = p;
                aslot = mine_slot;
                locked = true;
            } else if (pred >= 0 && k >= 1) {
                abit = p;
                aslot = pred;
            }
            res[e] = out;
        }
        td->bit0 = bit0 + advance;
        td->anchor_bit = abit;
        td->anchor_slot = aslot;
        td->locked = locked;
    }
    __syncthreads();
    for (int e = lane; e < ne; e += 64) {
        if (ownv[e] == DEAD) continue;
        const int v = res[e], slot = v & 0xffff;
        int32_t *row = slots + ((c0 + e / MAXB) * MAXB + e % MAXB) * TETRA_SLOT_FIELDS;
        row[TETRA_SLOT_TN] = v >= 0 ? slot % 4 + 1 : 0;
        row[TETRA_SLOT_FN] = v >= 0 ? slot / 4 % 18 + 1 : 0;
        row[TETRA_SLOT_MN] = v >= 0 ? slot / 72 + 1 : 0;
        row[TETRA_SLOT_FLAGS] = v >= 0 ? v >> 16 : 0;
    }
}

}  // namespace

void launch_mac_walk(tetra_ctx *ctx, size_t C, const int32_t *nburst, const int32_t *bursts, const int32_t *nblock,
                     const int32_t *blocks, const uint8_t *type1, int32_t *own, int32_t *npdu, int32_t *pdus) {
    hipLaunchKernelGGL(k_mac_walk, dim3(grid_for(C * MAC_LANES, MAC_BLOCK)), dim3(MAC_BLOCK), 0, ctx->stream, (int)C,
                       nburst, bursts, nblock, blocks, type1, own, npdu, pdus);
}

extern "C" int tetra_etsi_mac(tetra_ctx *ctx, const int32_t *nsym, size_t C, const int32_t *nburst,
                              const int32_t *bursts, const int32_t *nblock, const int32_t *blocks,
                              const uint8_t *type1, tetra_etsi_tdma *tdma, int32_t *slots, int32_t *npdu,
                              int32_t *pdus) {
    if (!ctx) return TETRA_E_INVALID;
    if (C == 0 || !nsym || !nburst || !bursts || !nblock || !blocks || !type1 || !tdma || !slots || !npdu || !pdus)
        return tetra_fail(ctx, TETRA_E_INVALID, "tetra_etsi_mac: C > 0 and every array");
    if (C > ((size_t)1 << 24)) return tetra_fail(ctx, TETRA_E_INVALID, "too many channels for one tetra_etsi_mac call (%zu)", C);
    Staging st(ctx);
    const int32_t *ns = (const int32_t *)st.in(nsym, C * 4);
    const int32_t *nb = (const int32_t *)st.in(nburst, C * 4);
    const int32_t *bu = (const int32_t *)st.in(bursts, C * MAXB * 2 * 4);
    const int32_t *nk = (const int32_t *)st.in(nblock, C * 4);
    const int32_t *bk = (const int32_t *)st.in(blocks, C * MAXJ * 4 * 4);
    const uint8_t *t1 = (const uint8_t *)st.in(type1, C * MAXJ * 268);
    tetra_etsi_tdma *td = (tetra_etsi_tdma *)st.inout(tdma, C * sizeof(tetra_etsi_tdma));
    // in/out, so that what the kernel does not write (rows past nburst, records past npdu) keeps the
    // caller's contents in host memory too
    int32_t *so = (int32_t *)st.inout(slots, C * MAXB * TETRA_SLOT_FIELDS * 4);
    int32_t *np = (int32_t *)st.out(npdu, C * MAXJ * 4);
    int32_t *po = (int32_t *)st.inout(pdus, C * MAXJ * MAXPDU * NF * 4);
    if (!ns || !nb || !bu || !nk || !bk || !t1 || !td || !so || !np || !po) return st.finish();
    {
        PROF(ctx, "etsi_mac");
        hipLaunchKernelGGL(k_etsi_mac, dim3(grid_for(C * MAC_LANES, MAC_BLOCK)), dim3(MAC_BLOCK), 0, ctx->stream, (int)C,
                           ns, nb, bu, nk, bk, t1, td, so, np, po);
    }
    return st.finish();
}

extern "C" int tetra_etsi_mac_groups(tetra_ctx *ctx, const int32_t *nsym, size_t C, size_t G, int64_t row_bits,
                                     int64_t tol_bits, int64_t advance, const int32_t *nburst, const int32_t *bursts,
                                     const int32_t *nblock, const int32_t *blocks, const uint8_t *type1,
                                     tetra_etsi_tdma *tdma, int32_t *keep, int32_t *slots, int32_t *npdu,
                                     int32_t *pdus) {
    if (!ctx) return TETRA_E_INVALID;
    if (C == 0 || !nsym || !nburst || !bursts || !nblock || !blocks || !type1 || !tdma || !keep || !slots || !npdu ||
        !pdus)
        return tetra_fail(ctx, TETRA_E_INVALID, "tetra_etsi_mac_groups: C > 0 and every array");
    if (G < 1 || G > (size_t)MAXG || C % G != 0 || row_bits < 0 || tol_bits < 0)
        return tetra_fail(ctx, TETRA_E_INVALID,
                          "tetra_etsi_mac_groups: 1 <= G <= %d rows per group dividing C, row_bits and tol_bits >= 0 "
                          "(C %zu, G %zu, row_bits %lld, tol_bits %lld)", MAXG, C, G, (long long)row_bits,
                          (long long)tol_bits);
    if (C > ((size_t)1 << 24)) return tetra_fail(ctx, TETRA_E_INVALID, "too many rows for one tetra_etsi_mac_groups call (%zu)", C);
    const size_t NG = C / G;
    Staging st(ctx);
    const int32_t *nb = (const int32_t *)st.in(nburst, C * 4);
    const int32_t *bu = (const int32_t *)st.in(bursts, C * MAXB * 2 * 4);
    const int32_t *nk = (const int32_t *)st.in(nblock, C * 4);
    const int32_t *bk = (const int32_t *)st.in(blocks, C * MAXJ * 4 * 4);
    const uint8_t *t1 = (const uint8_t *)st.in(type1, C * MAXJ * 268);
    tetra_etsi_tdma *td = (tetra_etsi_tdma *)st.inout(tdma, NG * sizeof(tetra_etsi_tdma));
    // in/out: what the kernels do not write keeps the caller's contents in host memory too
    int32_t *kp = (int32_t *)st.inout(keep, C * MAXB * 4);
    int32_t *so = (int32_t *)st.inout(slots, C * MAXB * TETRA_SLOT_FIELDS * 4);
    int32_t *np = (int32_t *)st.out(npdu, C * MAXJ * 4);
    int32_t *po = (int32_t *)st.inout(pdus, C * MAXJ * MAXPDU * NF * 4);
    int32_t *own = (int32_t *)ws(ctx, S_W0, C * MAXB * 4);
    if (!nb || !bu || !nk || !bk || !t1 || !td || !kp || !so || !np || !po || !own) return st.finish();
    {
        PROF(ctx, "etsi_mac_groups");
        hipLaunchKernelGGL(k_mac_walk, dim3(grid_for(C * MAC_LANES, MAC_BLOCK)), dim3(MAC_BLOCK), 0, ctx->stream, (int)C,
                           nb, bu, nk, bk, t1, own, np, po);
        hipLaunchKernelGGL(k_tdma_groups, dim3((unsigned)NG), dim3(64), 0, ctx->stream, (int)G, row_bits, tol_bits,
                           advance, nb, bu, own, td, kp, so);
    }
    return st.finish();
}
