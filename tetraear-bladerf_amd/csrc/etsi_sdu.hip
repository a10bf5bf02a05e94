// etsi_sdu.hip -- TM-SDUs of the ETSI chain's MAC PDUs and fragment reassembly on gfx950
// (tetra_etsi_sdu): the step after etsi_mac.hip, restated in tests/_etsi_sdu_model.py.
//
//   k_sdu_walk   16 lanes per row (4 rows per wave), lane j on block j, as k_etsi_mac: a block with
//                recorded PDUs is packed into an LDS bit row, the lane walks the optional elements of
//                each RESOURCE / END record by funnel reads, finds the fill bits on dwords, and cuts the
//                SDU's bytes from the row.  A row's lanes leave one flag: some record has ROLE != 0.
//   k_sdu_join   one wave per group of G rows: no flagged row and no active chain costs the flags, four
//                loads of `active` and bit0.  Otherwise the group's bursts are rank-sorted by position
//                (k_tdma_groups' order), and the wave walks them: every lane takes the same decision from
//                the chain heads in LDS, lane 0 writes it, the wave moves the bytes -- up to 34 appended
//                at an arbitrary bit offset, byte t of the destination from source bytes t - 1 and t.
#include "common.h"

namespace {

constexpr int MAXB = TETRA_ETSI_MAXB, MAXJ = TETRA_ETSI_MAXJ, MAXPDU = TETRA_ETSI_MAXPDU, NF = TETRA_PDU_FIELDS;
constexpr int NS = TETRA_SDU_FIELDS, ROWB = TETRA_SDU_ROW, MAXBYTES = TETRA_SDU_MAXBYTES, NCH = TETRA_FRAG_CHAINS;
constexpr int ND = TETRA_DONE_FIELDS;
constexpr int SDU_LANES = 16;    // lanes per row: one per block
constexpr int SDU_BLOCK = 256;   // 16 rows per workgroup
constexpr int WROW = 11;         // LDS dwords per lane: 268 bits in 9, one more for the funnel read; odd: no bank conflicts
constexpr int MAXG = 64, MAXE = MAXG * MAXB;

// n in 1..24 bits from bit `off` of an MSB-first bit row (bit p is bit 31 - (p & 31) of dword p >> 5)
__device__ __forceinline__ int field(const uint32_t *w, int off, int n) {
    const int q = off >> 5, s = off & 31;
    const uint64_t v = ((uint64_t)w[q] << 32) | w[q + 1];
    return (int)((uint32_t)(v >> (64 - s - n)) & ((1u << n) - 1));
}

// The first n1 bytes of a block (a multiple of 4) as bits, four per dword load; the dwords past n1 read 0.
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

// The optional elements in front of a TM-SDU, read from `pos` up to `end`.
struct Elems {
    int pos, end, status, elems, pg, chan;
    const uint32_t *w;
    __device__ __forceinline__ int take(int n) {   // the next n bits; past the end: malformed, 0
        if (status != TETRA_SDU_OK) return 0;
        if (pos + n > end) {
            status = TETRA_SDU_MALFORMED;
            return 0;
        }
        const int v = field(w, pos, n);
        pos += n;
        return v;
    }
    __device__ __forceinline__ bool ok() const { return status == TETRA_SDU_OK; }
    __device__ __forceinline__ void power_control() {
        if (take(1) && ok()) {
            const int v = take(4);
            if (ok()) elems |= 1, pg |= v;
        }
    }
    __device__ __forceinline__ void slot_granting() {
        if (take(1) && ok()) {
            const int v = take(8);
            if (ok()) elems |= 2, pg |= v << 8;
        }
    }
    __device__ __forceinline__ void channel_allocation() {
        if (!(take(1) && ok())) return;
        const int head = take(10);   // allocation type 2, timeslot 4, up/downlink 2, CLCH 1, cell change 1
        if (!ok()) return;
        elems |= 4;
        chan |= head;
        if (((head >> 2) & 3) == 0) {   // the augmented form
            status = TETRA_SDU_UNSUPPORTED;
            return;
        }
        const int carrier = take(12);
        if (!ok()) return;
        chan |= carrier << 16;
        if (take(1) && ok()) {
            const int ext = take(10);   // band 4, offset 2, duplex spacing 3, reverse operation 1
            if (ok()) elems |= 8, pg |= ext << 16;
        }
        const int mon = take(2);
        if (!ok()) return;
        chan |= mon << 28;
        if (mon == 0) {
            const int f18 = take(2);
            if (ok()) chan |= f18 << 10;
        }
    }
};

// The last 1 bit in [lo, hi) of the row, -1 when there is none: whole dwords, the lowest set bit.
__device__ __forceinline__ int last_one(const uint32_t *w, int lo, int hi) {
    if (hi <= lo) return -1;
    const int q0 = lo >> 5, q1 = (hi - 1) >> 5;
    for (int q = q1; q >= q0; --q) {
        uint32_t v = w[q];
        if (q == q1) v &= ~0u << (31 - ((hi - 1) & 31));
        if (q == q0) v &= ~0u >> (lo & 31);
        if (v) return 32 * q + 32 - __ffs((int)v);
    }
    return -1;
}

// Grid: 16 lanes per row, SDU_BLOCK / 16 rows per workgroup; the lanes past C idle.
__global__ __launch_bounds__(SDU_BLOCK) void k_sdu_walk(int C, const int32_t *__restrict__ nblock,
                                                        const int32_t *__restrict__ blocks,
                                                        const uint8_t *__restrict__ type1,
                                                        const int32_t *__restrict__ npdu,
                                                        const int32_t *__restrict__ pdus, int32_t *__restrict__ sdu,
                                                        uint8_t *__restrict__ sdu_data, int32_t *__restrict__ rowflag) {
    __shared__ uint32_t rows[SDU_BLOCK * WROW];
    const int tid = threadIdx.x, j = tid & (SDU_LANES - 1);
    const long ch = (long)blockIdx.x * (SDU_BLOCK / SDU_LANES) + tid / SDU_LANES;
    bool frag = false;   // this block holds a record with ROLE != 0
    if (ch < C && j < min(max(nblock[ch], 0), MAXJ)) {
        const size_t cj = (size_t)ch * MAXJ + j;
        const int kind = blocks[4 * cj], crc = blocks[4 * cj + 1];
        const int n = crc != 0 && kind >= TETRA_SCH_F && kind <= TETRA_BSCH ? min(max(npdu[cj], 0), MAXPDU) : 0;
        if (n > 0) {
            const int n1 = kind == TETRA_SCH_F ? 268 : kind == TETRA_SCH_HD ? 124 : 60;
            uint32_t *w = rows + tid * WROW;
            pack_block(type1 + cj * 268, n1, ((uintptr_t)type1 & 3) == 0, w);
            uint8_t *bytes = sdu_data + cj * ROWB;
            int at = 0;   // bytes of the block's row taken so far
            for (int q = 0; q < n; ++q) {
                const int32_t *r = pdus + (cj * MAXPDU + q) * NF;
                const int pk = r[TETRA_PDU_KIND], off = r[TETRA_PDU_OFFSET], nbits = r[TETRA_PDU_NBITS];
                const int hdr = r[TETRA_PDU_HDR_BITS], L = r[TETRA_PDU_LENGTH];
                const int role = pk == TETRA_PDU_RESOURCE ? (L == 63 ? TETRA_ROLE_FIRST : TETRA_ROLE_WHOLE)
                                 : pk == TETRA_PDU_FRAG   ? TETRA_ROLE_MIDDLE
                                 : pk == TETRA_PDU_END    ? TETRA_ROLE_LAST
                                                          : TETRA_ROLE_WHOLE;
                Elems e{0, 0, TETRA_SDU_NONE, 0, 0, 0, w};
                int so = 0, sn = 0;
                const bool carries = pk == TETRA_PDU_RESOURCE || pk == TETRA_PDU_FRAG || pk == TETRA_PDU_END;
                if (carries && r[TETRA_PDU_STATUS] == 0) {
                    if (off < 0 || nbits < 0 || off + nbits > n1 || hdr < 0 || hdr > nbits) {
                        e.status = TETRA_SDU_MALFORMED;   // not a record of this block: nothing is read
                    } else if (pk == TETRA_PDU_RESOURCE && r[TETRA_PDU_ENC] != 0) {
                        e.status = TETRA_SDU_ENCRYPTED;
                        so = off + hdr;
                        sn = nbits - hdr;
                    } else {
                        e.status = TETRA_SDU_OK;
                        e.pos = off + hdr;
                        e.end = off + nbits;
                        if (pk == TETRA_PDU_RESOURCE) e.power_control();
                        if (pk != TETRA_PDU_FRAG) {
                            e.slot_granting();
                            e.channel_allocation();
                        }
                        if (e.ok()) {
                            int stop = e.end;
                            if (r[TETRA_PDU_FILL] != 0) {
                                stop = last_one(w, e.pos, e.end);
                                if (stop < 0) e.status = TETRA_SDU_MALFORMED;
                            }
                            if (e.ok()) {
                                so = e.pos;
                                sn = stop - e.pos;
                            }
                        }
                    }
                }
                if (at + ((sn + 7) >> 3) > ROWB) {   // never for records that lie apart, as the walk's do
                    e.status = TETRA_SDU_MALFORMED;
                    so = sn = 0;
                }
                int32_t *o = sdu + (cj * MAXPDU + q) * NS;
                o[TETRA_SDU_STATUS] = e.status;
                o[TETRA_SDU_OFFSET] = so;
                o[TETRA_SDU_NBITS] = sn;
                o[TETRA_SDU_BYTE] = at;
                o[TETRA_SDU_ROLE] = role;
                o[TETRA_SDU_ELEMS] = e.elems;
                o[TETRA_SDU_POWER_GRANT] = e.pg;
                o[TETRA_SDU_CHAN] = e.chan;
                frag |= role != TETRA_ROLE_WHOLE;
                const int nby = (sn + 7) >> 3;
                for (int i = 0; i < nby; ++i) {
                    const int nb = min(8, sn - 8 * i);
                    bytes[at + i] = (uint8_t)(field(w, so + 8 * i, nb) << (8 - nb));
                }
                at += nby;
            }
        }
    }
    const unsigned long long any = __ballot(frag);
    if (ch < C && j == 0) rowflag[ch] = (int)((any >> ((tid & 63) & ~(SDU_LANES - 1))) & 0xffff) != 0;
}

struct Head {   // a chain's head in LDS
    int64_t last_bit;
    int32_t active, ssi, addr_type, aux, enc, nbits, nfrag, span, fed;
};

// floor((d + 255) / 510) for any d of an int64 stream
__device__ __forceinline__ int64_t slots_of(int64_t d) {
    const int64_t x = d + 255;
    return x >= 0 ? x / 510 : -((509 - x) / 510);
}

// One wave per group.  Entry e = row * MAXB + b, so the order (pos, row, b) is (pos, e).
// The workgroup must stay one wave of 64: the walk's paths without a barrier (ROLE 0, a first fragment
// with a bad status) and the expiry's writes by lanes 0..3 rely on the lanes running in lockstep.
__global__ __launch_bounds__(64) void k_sdu_join(int G, int64_t row_bits, int64_t advance, int gap_slots, int maxd,
                                                 const int32_t *__restrict__ nsym, const int32_t *__restrict__ nburst,
                                                 const int32_t *__restrict__ bursts,
                                                 const int32_t *__restrict__ nblock,
                                                 const int32_t *__restrict__ blocks, const int32_t *__restrict__ npdu,
                                                 const int32_t *__restrict__ pdus, const int32_t *__restrict__ keep,
                                                 const int32_t *__restrict__ rowflag, const int32_t *sdu,
                                                 const uint8_t *sdu_data, tetra_etsi_frag *frag, int32_t *ndone,
                                                 int32_t *done, uint8_t *done_data) {
    __shared__ int64_t pos[MAXE];
    __shared__ uint16_t order[MAXE];   // rank -> entry
    __shared__ uint8_t live[MAXE];
    __shared__ Head head[NCH];
    __shared__ int nlive, dropped, orphans, count;
    const int lane = threadIdx.x, ne = G * MAXB;
    const size_t g = blockIdx.x, c0 = g * G;
    tetra_etsi_frag *fs = frag + g;
    const int64_t adv = nsym ? 2 * (int64_t)max(nsym[c0] - 1, 0) : advance;

    // nothing to join and nothing waiting: the flags, four loads and bit0
    int busy = lane < NCH ? fs->chain[lane].active != 0 : 0;
    for (int i = lane; i < G; i += 64) busy |= rowflag[c0 + i] != 0;
    if (__ballot(busy) == 0) {
        if (lane == 0) {
            fs->bit0 += adv;
            ndone[g] = 0;
        }
        return;
    }

    if (lane < NCH) {
        const tetra_etsi_frag_chain *c = fs->chain + lane;
        head[lane] = Head{c->last_bit, c->active != 0, c->ssi, c->addr_type, c->aux, c->enc, c->nbits, c->nfrag, c->span, c->fed};
    }
    if (lane == 0) {
        nlive = 0;
        dropped = fs->dropped;
        orphans = fs->orphans;
        count = 0;
    }
    __syncthreads();
    int mine = 0;
    for (int e = lane; e < ne; e += 64) {
        const int i = e / MAXB, b = e % MAXB;
        const bool lv = b < min(max(nburst[c0 + i], 0), MAXB);
        pos[e] = lv ? (int64_t)((uint64_t)i * (uint64_t)row_bits) + bursts[((c0 + i) * MAXB + b) * 2] : 0;
        live[e] = lv;
        mine += lv;
    }
    if (mine) atomicAdd(&nlive, mine);
    __syncthreads();
    for (int e = lane; e < ne; e += 64) {   // rank sort: exact and stable
        if (!live[e]) continue;
        const int64_t pe = pos[e];
        int rank = 0;
#pragma unroll 8
        for (int f = 0; f < ne; ++f) {
            const int64_t pf = pos[f];
            rank += (int)live[f] & ((int)(pf < pe) | ((int)(pf == pe) & (int)(f < e)));
        }
        order[rank] = (uint16_t)e;
    }
    __syncthreads();

    const int n = nlive;
    const int64_t bit0 = fs->bit0;
    for (int r = 0; r < n; ++r) {   // every lane walks alike; lane 0 writes the heads, the wave moves bytes
        const int e = order[r], b = e % MAXB;
        const size_t c = c0 + e / MAXB;
        if (keep && keep[c * MAXB + b] == 0) continue;
        const int64_t p = bit0 + pos[e];
        if (lane < NCH && head[lane].active && slots_of(p - head[lane].last_bit) > gap_slots) {   // rule 1
            head[lane].active = 0;
            atomicAdd(&dropped, 1);
        }
        __syncthreads();
        const int nk = min(max(nblock[c], 0), MAXJ);
        for (int j = 0; j < nk; ++j) {
            const size_t cj = c * MAXJ + j;
            const int kind = blocks[4 * cj], crc = blocks[4 * cj + 1];
            if (blocks[4 * cj + 2] != b || crc == 0 || kind < TETRA_SCH_F || kind > TETRA_BSCH) continue;
            const int np = min(max(npdu[cj], 0), MAXPDU);
            for (int q = 0; q < np; ++q) {
                const int32_t *s = sdu + (cj * MAXPDU + q) * NS;
                const int role = s[TETRA_SDU_ROLE];
                if (role == TETRA_ROLE_WHOLE) continue;
                const int status = s[TETRA_SDU_STATUS], sn = s[TETRA_SDU_NBITS];
                const uint8_t *src = sdu_data + cj * ROWB + s[TETRA_SDU_BYTE];
                int same = 0;   // rule 2: the chains on this burst's timeslot
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    const int64_t d = p - head[i].last_bit, k = slots_of(d), rr = d - 510 * k;
                    if (head[i].active && k >= 0 && (k & 3) == 0 && rr >= -TETRA_TDMA_TOL && rr <= TETRA_TDMA_TOL)
                        same |= 1 << i;
                }
                if (role == TETRA_ROLE_FIRST) {
                    if (status != TETRA_SDU_OK) continue;   // rule 5
                    int act = 0, oldest = 0;
#pragma unroll
                    for (int i = 0; i < NCH; ++i) {
                        act |= (head[i].active && !((same >> i) & 1)) << i;
                        if (head[i].last_bit < head[oldest].last_bit) oldest = i;
                    }
                    const int ndrop = __popc(same) + (act == (1 << NCH) - 1);
                    const int t = act == (1 << NCH) - 1 ? oldest : __ffs(~act) - 1;
                    const int32_t *pr = pdus + (cj * MAXPDU + q) * NF;
                    const int ssi = pr[TETRA_PDU_SSI], at = pr[TETRA_PDU_ADDR_TYPE], aux = pr[TETRA_PDU_AUX], enc = pr[TETRA_PDU_ENC];
                    __syncthreads();
                    if (lane == 0) {
#pragma unroll
                        for (int i = 0; i < NCH; ++i)
                            if ((same >> i) & 1) head[i].active = 0;
                        dropped += ndrop;
                        head[t] = Head{p, 1, ssi, at, aux, enc, sn, 1, 0, 1};
                    }
                    if (lane < ((sn + 7) >> 3)) fs->chain[t].data[lane] = src[lane];
                    __syncthreads();
                    continue;
                }
                // rule 4 / 5: a middle or last fragment
                const int t = same ? __ffs(same) - 1 : -1;
                if (status != TETRA_SDU_OK || t < 0) {
                    __syncthreads();
                    if (lane == 0) orphans += 1;
                    __syncthreads();
                    continue;
                }
                const int n0 = head[t].nbits;
                if (n0 + sn > 8 * MAXBYTES) {
                    __syncthreads();
                    if (lane == 0) {
                        head[t].active = 0;
                        dropped += 1;
                    }
                    __syncthreads();
                    continue;
                }
                const int sh = n0 & 7, q0 = n0 >> 3, nsrc = (sn + 7) >> 3, ndst = (sh + sn + 7) >> 3;
                uint8_t *dst = fs->chain[t].data;
                __syncthreads();   // the chain's earlier bytes, written by other lanes, are visible
                if (lane < ndst) {
                    const unsigned hi = lane == 0 ? (sh ? dst[q0] >> (8 - sh) : 0u) : src[lane - 1];
                    const unsigned lo = lane < nsrc ? src[lane] : 0u;
                    dst[q0 + lane] = (uint8_t)(((hi << 8 | lo) >> sh) & 0xff);
                }
                const Head h = head[t];
                const int k = (int)slots_of(p - h.last_bit), total = n0 + sn;
                const int slot = count;
                __syncthreads();
                if (lane == 0) {
                    head[t].nbits = total;
                    head[t].nfrag = h.nfrag + 1;
                    head[t].span = h.span + k;
                    head[t].fed = h.fed + (k > 0);
                    head[t].last_bit = p;
                    if (role == TETRA_ROLE_LAST) {
                        head[t].active = 0;
                        count = slot + 1;
                    }
                }
                if (role == TETRA_ROLE_LAST && slot < maxd) {
                    const size_t di = g * (size_t)maxd + slot;
                    if (lane == 0) {
                        int32_t *o = done + di * ND;
                        const int span = h.span + k, fed = h.fed + (k > 0);
                        o[TETRA_DONE_ROW] = (int)c;
                        o[TETRA_DONE_BURST] = b;
                        o[TETRA_DONE_BLOCK] = j;
                        o[TETRA_DONE_PDU] = q;
                        o[TETRA_DONE_SSI] = h.ssi;
                        o[TETRA_DONE_ADDR_TYPE] = h.addr_type;
                        o[TETRA_DONE_AUX] = h.aux;
                        o[TETRA_DONE_ENC] = h.enc;
                        o[TETRA_DONE_NBITS] = total;
                        o[TETRA_DONE_NFRAG] = h.nfrag + 1;
                        o[TETRA_DONE_SPAN] = span;
                        o[TETRA_DONE_FED] = fed;
                        o[TETRA_DONE_GAPS] = span / 4 + 1 - fed;
                    }
                    const int nby = (total + 7) >> 3;
                    for (int i = lane; i < nby; i += 64) done_data[di * MAXBYTES + i] = dst[i];
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    if (lane < NCH) {
        tetra_etsi_frag_chain *c = fs->chain + lane;
        const Head h = head[lane];
        c->last_bit = h.last_bit;
        c->active = h.active;
        c->ssi = h.ssi;
        c->addr_type = h.addr_type;
        c->aux = h.aux;
        c->enc = h.enc;
        c->nbits = h.nbits;
        c->nfrag = h.nfrag;
        c->span = h.span;
        c->fed = h.fed;
    }
    if (lane == 0) {
        fs->bit0 = bit0 + adv;
        fs->dropped = dropped;
        fs->orphans = orphans;
        ndone[g] = count;
    }
}

}  // namespace

extern "C" int tetra_etsi_sdu(tetra_ctx *ctx, const int32_t *nsym, size_t C, size_t G, int64_t row_bits, int64_t advance,
                              int32_t gap_slots, const int32_t *nburst, const int32_t *bursts, const int32_t *nblock,
                              const int32_t *blocks, const uint8_t *type1, const int32_t *npdu, const int32_t *pdus,
                              const int32_t *keep, int32_t *sdu, uint8_t *sdu_data, tetra_etsi_frag *frag, int32_t maxd,
                              int32_t *ndone, int32_t *done, uint8_t *done_data) {
    if (!ctx) return TETRA_E_INVALID;
    const bool streaming = G == 1 && row_bits == 0 && !keep;
    if (C == 0 || !nburst || !bursts || !nblock || !blocks || !type1 || !npdu || !pdus || !sdu || !sdu_data || !frag ||
        !ndone || (streaming && !nsym) || (maxd > 0 && (!done || !done_data)))
        return tetra_fail(ctx, TETRA_E_INVALID, "tetra_etsi_sdu: C > 0 and every array but keep (nsym in the streaming form)");
    if (G < 1 || G > (size_t)MAXG || C % G != 0 || row_bits < 0 || gap_slots < 0 || maxd < 0)
        return tetra_fail(ctx, TETRA_E_INVALID,
                          "tetra_etsi_sdu: 1 <= G <= %d rows per group dividing C, row_bits, gap_slots and maxd >= 0 "
                          "(C %zu, G %zu, row_bits %lld, gap_slots %d, maxd %d)", MAXG, C, G, (long long)row_bits,
                          (int)gap_slots, (int)maxd);
    if (C > ((size_t)1 << 24)) return tetra_fail(ctx, TETRA_E_INVALID, "too many rows for one tetra_etsi_sdu call (%zu)", C);
    const size_t NG = C / G;
    Staging st(ctx);
    // the small host arrays travel as one staged input (five staged inputs in all)
    Staging::Part small[] = {{streaming ? nsym : nullptr, C}, {nburst, C}, {nblock, C}, {npdu, C * MAXJ}, {keep, C * MAXB}};
    if (!st.pack(small)) return st.finish();
    const int32_t *ns = (const int32_t *)small[0].p, *nb = (const int32_t *)small[1].p, *nk = (const int32_t *)small[2].p,
                  *np = (const int32_t *)small[3].p, *kp = (const int32_t *)small[4].p;
    const int32_t *bu = (const int32_t *)st.in(bursts, C * MAXB * 2 * 4);
    const int32_t *bk = (const int32_t *)st.in(blocks, C * MAXJ * 4 * 4);
    const uint8_t *t1 = (const uint8_t *)st.in(type1, C * MAXJ * 268);
    const int32_t *pd = (const int32_t *)st.in(pdus, C * MAXJ * MAXPDU * NF * 4);
    // in/out: what the kernels do not write keeps the caller's contents in host memory too
    int32_t *so = (int32_t *)st.inout(sdu, C * MAXJ * MAXPDU * NS * 4);
    uint8_t *sd = (uint8_t *)st.inout(sdu_data, C * MAXJ * ROWB);
    tetra_etsi_frag *fr = (tetra_etsi_frag *)st.inout(frag, NG * sizeof(tetra_etsi_frag));
    int32_t *nd = (int32_t *)st.out(ndone, NG * 4);
    int32_t *dn = maxd > 0 ? (int32_t *)st.inout(done, NG * (size_t)maxd * ND * 4) : nullptr;
    uint8_t *dd = maxd > 0 ? (uint8_t *)st.inout(done_data, NG * (size_t)maxd * MAXBYTES) : nullptr;
    int32_t *flag = (int32_t *)ws(ctx, S_W0, C * 4);
    if (!bu || !bk || !t1 || !pd || !so || !sd || !fr || !nd || (maxd > 0 && (!dn || !dd)) || !flag) return st.finish();
    {
        PROF(ctx, "etsi_sdu");
        hipLaunchKernelGGL(k_sdu_walk, dim3(grid_for(C * SDU_LANES, SDU_BLOCK)), dim3(SDU_BLOCK), 0, ctx->stream, (int)C,
                           nk, bk, t1, np, pd, so, sd, flag);
        hipLaunchKernelGGL(k_sdu_join, dim3((unsigned)NG), dim3(64), 0, ctx->stream, (int)G, row_bits, advance,
                           (int)gap_slots, (int)maxd, ns, nb, bu, nk, bk, np, pd, kp, flag, so, sd, fr, nd, dn, dd);
    }
    return st.finish();
}
