// etsi_assign.hip -- channel allocations followed per carrier on gfx950 (tetra_etsi_assign): the step after
// etsi_sdu.hip, restated in tests/_etsi_assign_model.py.
//
//   k_assign_scan    16 lanes per row (4 rows per wave), lane j on block j, as k_sdu_walk: a row's lanes leave
//                    one flag -- some recorded PDU of a kept burst is an event -- and lanes 0..7 write the
//                    ta rows an idle carrier has (STATE 0 or -1).  Thread 0 clears the list's counter.
//   k_assign_events  one wave per group: no flagged row costs the flags and nev.  Otherwise the group's bursts
//                    are rank-sorted by position (k_sdu_join's order, restated), every lane walks them alike
//                    and lane 0 writes the event records; a recorded event that can apply somewhere is
//                    appended to one compact list (target key, time, source, ordinal) by an atomic counter.
//                    The append order does not matter: the follower orders by (time, source, ordinal).
//   k_assign_follow  one wave per group: no active entry and no listed event with the group's key costs four
//                    loads of `active`, the counter and bit0.  Otherwise the bursts are rank-sorted, and the
//                    wave merges them with the group's events, taken one at a time as the smallest listed one
//                    behind the last (a scan of the list per event: exact for any number of them); every
//                    lane takes the same decision from the entries in LDS, lane 0 writes them.
#include "common.h"

namespace {

constexpr int MAXB = TETRA_ETSI_MAXB, MAXJ = TETRA_ETSI_MAXJ, MAXPDU = TETRA_ETSI_MAXPDU, NF = TETRA_PDU_FIELDS;
constexpr int NS = TETRA_SDU_FIELDS, ND = TETRA_DONE_FIELDS, NE = TETRA_AE_FIELDS, NT = TETRA_TA_FIELDS;
constexpr int NSL = TETRA_SLOT_FIELDS, NQ = TETRA_TQ_FIELDS;
constexpr int SCAN_LANES = 16;    // lanes per row: one per block
constexpr int SCAN_BLOCK = 256;   // 16 rows per workgroup
constexpr int MAXG = 64, MAXE = MAXG * MAXB;
static_assert(MAXJ == SCAN_LANES && MAXB <= SCAN_LANES && NT == 8 && NE == 16 && sizeof(tetra_etsi_assign_state) == 208,
              "record layout");

struct Listed {   // an entry of the compact list
    int64_t T;
    int32_t src, ord;
};

// floor((d + 255) / 510) for any d of an int64 stream (etsi_sdu.hip's)
__device__ __forceinline__ int64_t slots_of(int64_t d) {
    const int64_t x = d + 255;
    return x >= 0 ? x / 510 : -((509 - x) / 510);
}

// is PDU q of block cj an event: ELEMS bit 2, STATUS ok, MAC-RESOURCE or MAC-END
__device__ __forceinline__ bool is_event(const int32_t *__restrict__ sdu, const int32_t *__restrict__ pdus, size_t cj, int q) {
    const int32_t *s = sdu + (cj * MAXPDU + q) * NS;
    if (!(s[TETRA_SDU_ELEMS] & 4) || s[TETRA_SDU_STATUS] != TETRA_SDU_OK) return false;
    const int pk = pdus[(cj * MAXPDU + q) * NF + TETRA_PDU_KIND];
    return pk == TETRA_PDU_RESOURCE || pk == TETRA_PDU_END;
}

// does burst b of row c take part in the follower's walk
__device__ __forceinline__ bool takes_part(const int32_t *keep, const int32_t *slots, const int32_t *tq, size_t cb, int &tn) {
    tn = slots ? slots[cb * NSL + TETRA_SLOT_TN] : 0;
    if (keep && keep[cb] == 0) return false;
    if (tn < 1 || tn > 4) return false;
    return !tq || tq[cb * NQ + TETRA_TQ_CLASS] >= 0;
}

// Grid: 16 lanes per row, SCAN_BLOCK / 16 rows per workgroup; the lanes past C idle.
__global__ __launch_bounds__(SCAN_BLOCK) void k_assign_scan(int C, const int32_t *__restrict__ nburst,
                                                            const int32_t *__restrict__ nblock,
                                                            const int32_t *__restrict__ blocks,
                                                            const int32_t *__restrict__ npdu,
                                                            const int32_t *__restrict__ pdus,
                                                            const int32_t *__restrict__ keep,
                                                            const int32_t *__restrict__ slots,
                                                            const int32_t *__restrict__ tq,
                                                            const int32_t *__restrict__ sdu, int32_t *__restrict__ rowflag,
                                                            int32_t *__restrict__ count, int32_t *__restrict__ ta) {
    const int tid = threadIdx.x, j = tid & (SCAN_LANES - 1);
    const long ch = (long)blockIdx.x * (SCAN_BLOCK / SCAN_LANES) + tid / SCAN_LANES;
    if (blockIdx.x == 0 && tid == 0) *count = 0;
    bool hit = false;
    if (ch < C) {
        const int nb = min(max(nburst[ch], 0), MAXB);
        if (j < min(max(nblock[ch], 0), MAXJ)) {
            const size_t cj = (size_t)ch * MAXJ + j;
            const int kind = blocks[4 * cj], crc = blocks[4 * cj + 1], b = blocks[4 * cj + 2];
            const int n = crc != 0 && kind >= TETRA_SCH_F && kind <= TETRA_BSCH ? min(max(npdu[cj], 0), MAXPDU) : 0;
            if (n > 0 && b >= 0 && b < nb && !(keep && keep[(size_t)ch * MAXB + b] == 0))
                for (int q = 0; q < n; ++q) hit |= is_event(sdu, pdus, cj, q);
        }
        if (j < nb) {   // the ta row of an idle carrier's burst: the follower rewrites it where an entry is active
            const size_t cb = (size_t)ch * MAXB + j;
            int tn;
            const bool part = takes_part(keep, slots, tq, cb, tn);
            int4 *o = reinterpret_cast<int4 *>(ta + cb * NT);   // 32-byte records of a hipMalloc'd or caller array
            if (((uintptr_t)ta & 15) == 0) {
                o[0] = part ? make_int4(0, -1, 0, -1) : make_int4(-1, 0, 0, 0);
                o[1] = part ? make_int4(-1, 0, 0, 0) : make_int4(0, 0, 0, 0);
            } else {
                int32_t *w = ta + cb * NT;
#pragma unroll
                for (int i = 0; i < NT; ++i)
                    w[i] = !part ? (i == TETRA_TA_STATE ? -1 : 0)
                                 : (i == TETRA_TA_SSI || i == TETRA_TA_AUX || i == TETRA_TA_SRC_KEY ? -1 : 0);
            }
        }
    }
    const unsigned long long any = __ballot(hit);
    if (ch < C && j == 0) rowflag[ch] = (int)((any >> ((tid & 63) & ~(SCAN_LANES - 1))) & 0xffff) != 0;
}

// The group's live bursts rank-sorted by (pos, row, b): entry e = row * MAXB + b, so the order is (pos, e).
// Exact and stable; k_sdu_join's sort restated.  Returns the number of live bursts.  One wave of 64.
__device__ __forceinline__ int sort_bursts(int G, int64_t row_bits, size_t c0, const int32_t *__restrict__ nburst,
                                           const int32_t *__restrict__ bursts, int64_t *pos, uint16_t *order,
                                           uint8_t *live, int *nlive) {
    const int lane = threadIdx.x, ne = G * MAXB;
    if (lane == 0) *nlive = 0;
    __syncthreads();
    int mine = 0;
    for (int e = lane; e < ne; e += 64) {
        const int i = e / MAXB, b = e % MAXB;
        const bool lv = b < min(max(nburst[c0 + i], 0), MAXB);
        pos[e] = lv ? (int64_t)((uint64_t)i * (uint64_t)row_bits) + bursts[((c0 + i) * MAXB + b) * 2] : 0;
        live[e] = lv;
        mine += lv;
    }
    if (mine) atomicAdd(nlive, mine);
    __syncthreads();
    for (int e = lane; e < ne; e += 64) {
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
    return *nlive;
}

// the frequency offset of a key's two low bits, and of the extended bits' offset field
__device__ __forceinline__ int key_offset(int o) { return o == 3 ? -1 : o; }
__device__ __forceinline__ int ext_offset(int o) { return o == 2 ? -1 : o == 3 ? 2 : o; }

// One wave per group; every lane walks alike, lane 0 writes.
__global__ __launch_bounds__(64) void k_assign_events(int G, int64_t row_bits, int maxe, int maxd, int cap,
                                                      const int32_t *__restrict__ nburst, const int32_t *__restrict__ bursts,
                                                      const int32_t *__restrict__ nblock, const int32_t *__restrict__ blocks,
                                                      const int32_t *__restrict__ npdu, const int32_t *__restrict__ pdus,
                                                      const int32_t *__restrict__ keep, const int32_t *__restrict__ slots,
                                                      const int32_t *__restrict__ sdu, const int32_t *__restrict__ ndone,
                                                      const int32_t *__restrict__ done, const int32_t *__restrict__ row_key,
                                                      const int32_t *__restrict__ rowflag,
                                                      const tetra_etsi_assign_state *__restrict__ state,
                                                      int32_t *__restrict__ nev, int32_t *__restrict__ ev,
                                                      int32_t *count, int32_t *__restrict__ ckey, Listed *__restrict__ clist) {
    __shared__ int64_t pos[MAXE];
    __shared__ uint16_t order[MAXE];
    __shared__ uint8_t live[MAXE];
    __shared__ int nlive;
    const int lane = threadIdx.x;
    const size_t g = blockIdx.x, c0 = g * G;
    int busy = 0;
    for (int i = lane; i < G; i += 64) busy |= rowflag[c0 + i] != 0;
    if (__ballot(busy) == 0) {
        if (lane == 0) nev[g] = 0;
        return;
    }
    const int n = sort_bursts(G, row_bits, c0, nburst, bursts, pos, order, live, &nlive);
    const int64_t bit0 = state[g].bit0;
    const int own = row_key ? row_key[g] : -1;
    const int nd = maxd > 0 ? min(max(ndone[g], 0), maxd) : 0;
    int k = 0;
    for (int r = 0; r < n; ++r) {
        const int e = order[r], b = e % MAXB;
        const size_t c = c0 + e / MAXB, cb = c * MAXB + b;
        if (keep && keep[cb] == 0) continue;
        const int64_t p = bit0 + pos[e];
        const int nk = min(max(nblock[c], 0), MAXJ);
        for (int j = 0; j < nk; ++j) {
            const size_t cj = c * MAXJ + j;
            const int kind = blocks[4 * cj], crc = blocks[4 * cj + 1];
            if (blocks[4 * cj + 2] != b || crc == 0 || kind < TETRA_SCH_F || kind > TETRA_BSCH) continue;
            const int np = min(max(npdu[cj], 0), MAXPDU);
            for (int q = 0; q < np; ++q) {
                if (!is_event(sdu, pdus, cj, q)) continue;
                const int32_t *s = sdu + (cj * MAXPDU + q) * NS, *pr = pdus + (cj * MAXPDU + q) * NF;
                const int pk = pr[TETRA_PDU_KIND];
                const int head = s[TETRA_SDU_CHAN] & 0x3ff, carrier = (s[TETRA_SDU_CHAN] >> 16) & 0xfff;
                const bool extd = (s[TETRA_SDU_ELEMS] & 8) != 0;
                const int ext = extd ? (s[TETRA_SDU_POWER_GRANT] >> 16) & 0x3ff : -1;
                int target;
                if (extd) target = (ext >> 6) * 16000 + carrier * 4 + ext_offset((ext >> 4) & 3);
                else if (own < 0) target = -1;
                else {
                    const int off = key_offset(own & 3);
                    target = (own - off) / 16000 * 16000 + carrier * 4 + off;
                }
                int ssi = -1, at = -1, aux = -1;
                if (pk == TETRA_PDU_RESOURCE) {
                    ssi = pr[TETRA_PDU_SSI];
                    at = pr[TETRA_PDU_ADDR_TYPE];
                    aux = pr[TETRA_PDU_AUX];
                } else {
                    for (int i = 0; i < nd; ++i) {
                        const int32_t *d = done + (g * (size_t)maxd + i) * ND;
                        if (d[TETRA_DONE_ROW] == (int)c && d[TETRA_DONE_BURST] == b && d[TETRA_DONE_BLOCK] == j &&
                            d[TETRA_DONE_PDU] == q) {
                            ssi = d[TETRA_DONE_SSI];
                            at = d[TETRA_DONE_ADDR_TYPE];
                            aux = d[TETRA_DONE_AUX];
                            break;
                        }
                    }
                }
                if (k < maxe && lane == 0) {
                    int32_t *o = ev + (g * (size_t)maxe + k) * NE;
                    o[TETRA_AE_ROW] = (int)c;
                    o[TETRA_AE_BURST] = b;
                    o[TETRA_AE_BLOCK] = j;
                    o[TETRA_AE_PDU] = q;
                    o[TETRA_AE_KIND] = pk;
                    o[TETRA_AE_HEAD] = head;
                    o[TETRA_AE_CARRIER] = carrier;
                    o[TETRA_AE_EXT] = ext;
                    o[TETRA_AE_TARGET] = target;
                    o[TETRA_AE_P_LO] = (int32_t)(uint32_t)((uint64_t)p & 0xffffffffu);
                    o[TETRA_AE_P_HI] = (int32_t)(p >> 32);
                    o[TETRA_AE_TN] = slots ? slots[cb * NSL + TETRA_SLOT_TN] : 0;
                    o[TETRA_AE_FN] = slots ? slots[cb * NSL + TETRA_SLOT_FN] : 0;
                    o[TETRA_AE_SSI] = ssi;
                    o[TETRA_AE_ADDR_TYPE] = at;
                    o[TETRA_AE_AUX] = aux;
                    const int ud = (head >> 2) & 3;
                    if (target >= 0 && (ud == 1 || ud == 3) && ((head >> 4) & 15) != 0) {
                        const int at_list = atomicAdd(count, 1);
                        if (at_list < cap) {   // cap bounds what a call can record: never exceeded
                            ckey[at_list] = target;
                            clist[at_list] = Listed{p, (int32_t)g, k};
                        }
                    }
                }
                ++k;
            }
        }
    }
    if (lane == 0) nev[g] = k;
}

struct Entry {   // a timeslot's entry in LDS
    int64_t since, last;
    int32_t active, ssi, addr_type, aux, src_key, head, nalloc, idle;
};

// One wave per group.  The workgroup must stay one wave of 64: every lane walks alike.
__global__ __launch_bounds__(64) void k_assign_follow(int G, int64_t row_bits, int64_t advance, int hold_slots,
                                                      int idle_max, int shared_clock, int maxe, int cap,
                                                      const int32_t *__restrict__ nsym, const int32_t *__restrict__ nburst,
                                                      const int32_t *__restrict__ bursts, const int32_t *__restrict__ keep,
                                                      const int32_t *__restrict__ slots, const int32_t *__restrict__ tq,
                                                      const int32_t *__restrict__ row_key, const int32_t *__restrict__ ev,
                                                      const int32_t *__restrict__ count, const int32_t *__restrict__ ckey,
                                                      const Listed *__restrict__ clist, tetra_etsi_assign_state *state,
                                                      int32_t *ta) {
    __shared__ int64_t pos[MAXE];
    __shared__ uint16_t order[MAXE];
    __shared__ uint8_t live[MAXE];
    __shared__ Entry ent[4];
    __shared__ int64_t redT[64];
    __shared__ int32_t redS[64], redO[64];
    __shared__ int nlive, expired, released;
    const int lane = threadIdx.x;
    const size_t g = blockIdx.x, c0 = g * G;
    tetra_etsi_assign_state *st = state + g;
    const int64_t adv = nsym ? 2 * (int64_t)max(nsym[c0] - 1, 0) : advance;
    const int mykey = row_key ? row_key[g] : -1;
    const int nl = mykey >= 0 ? min(max(*count, 0), cap) : 0;

    // no entry active and no listed event for this carrier: four loads, the counter and bit0
    int busy = lane < 4 ? st->slot[lane].active != 0 : 0;
    for (int i = lane; i < nl; i += 64) busy |= ckey[i] == mykey && (shared_clock || clist[i].src == (int)g);
    if (__ballot(busy) == 0) {
        if (lane == 0) st->bit0 += adv;
        return;
    }

    if (lane < 4) {
        const tetra_etsi_assign_slot *s = st->slot + lane;
        ent[lane] = Entry{s->since, s->last, s->active != 0, s->ssi, s->addr_type, s->aux, s->src_key, s->head, s->nalloc, s->idle};
    }
    if (lane == 0) {
        expired = st->expired;
        released = st->released;
    }
    const int n = sort_bursts(G, row_bits, c0, nburst, bursts, pos, order, live, &nlive);   // (its barriers cover the above)
    const int64_t bit0 = st->bit0;

    // the smallest listed event of this carrier behind (pT, pS, pO); have = false: the smallest of all
    bool have = false, more = nl > 0;
    int64_t pT = 0, nT = 0;
    int pS = 0, pO = 0, nS = 0, nO = 0;
    auto next_event = [&]() {
        bool f = false;
        int64_t bT = 0;
        int bS = 0, bO = 0;
        for (int i = lane; i < nl; i += 64) {
            if (ckey[i] != mykey) continue;
            const Listed L = clist[i];
            if (!shared_clock && L.src != (int)g) continue;
            if (have && !(L.T > pT || (L.T == pT && (L.src > pS || (L.src == pS && L.ord > pO))))) continue;
            if (!f || L.T < bT || (L.T == bT && (L.src < bS || (L.src == bS && L.ord < bO)))) f = true, bT = L.T, bS = L.src, bO = L.ord;
        }
        redT[lane] = bT;
        redS[lane] = f ? bS : -1;   // a source group is never negative
        redO[lane] = bO;
        __syncthreads();
        bool any = false;
        for (int i = 0; i < 64; ++i) {
            const int s = redS[i];
            if (s < 0) continue;
            const int64_t t = redT[i];
            const int o = redO[i];
            if (!any || t < nT || (t == nT && (s < nS || (s == nS && o < nO)))) any = true, nT = t, nS = s, nO = o;
        }
        __syncthreads();
        more = any;
    };
    auto apply_event = [&]() {
        const int32_t *e = ev + ((size_t)nS * (size_t)maxe + nO) * NE;
        const int head = e[TETRA_AE_HEAD], ssi = e[TETRA_AE_SSI], at = e[TETRA_AE_ADDR_TYPE], aux = e[TETRA_AE_AUX];
        const int skey = row_key[nS], map = (head >> 4) & 15;
        if (lane == 0) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (!((map >> (3 - t)) & 1)) continue;
                Entry &d = ent[t];
                if (!d.active) d.active = 1, d.since = nT, d.nalloc = 0, d.idle = 0;
                d.last = nT;
                d.nalloc += 1;
                d.ssi = ssi;
                d.addr_type = at;
                d.aux = aux;
                d.head = head;
                d.src_key = skey;
            }
        }
        __syncthreads();
        have = true, pT = nT, pS = nS, pO = nO;
    };
    if (more) next_event();

    for (int r = 0; r < n; ++r) {
        const int e = order[r], b = e % MAXB;
        const size_t cb = (c0 + e / MAXB) * MAXB + b;
        const int64_t p = bit0 + pos[e];
        while (more && nT < p) {   // an event at T comes behind every burst with p <= T
            apply_event();
            next_event();
        }
        int tn;
        if (!takes_part(keep, slots, tq, cb, tn)) continue;   // (its ta row is k_assign_scan's)
        const Entry d = ent[tn - 1];
        const bool exp = d.active && slots_of(p - d.last) > hold_slots;
        const bool act = d.active && !exp;
        if (lane < NT) {
            const int age = (int32_t)(uint32_t)((uint64_t)slots_of(p - d.since) & 0xffffffffu);
            const int on[NT] = {1, d.ssi, d.addr_type, d.aux, d.src_key, d.nalloc, d.idle, age};
            const int off[NT] = {0, -1, 0, -1, -1, 0, 0, 0};
            int v = 0;
#pragma unroll
            for (int i = 0; i < NT; ++i)
                if (lane == i) v = act ? on[i] : off[i];
            ta[cb * NT + lane] = v;
        }
        const int cls = tq ? tq[cb * NQ + TETRA_TQ_CLASS] : -1;
        const int fn = slots[cb * NSL + TETRA_SLOT_FN];   // slots is given: the burst takes part
        __syncthreads();   // every lane has read the entry
        if (lane == 0) {
            Entry &w = ent[tn - 1];
            if (exp) w.active = 0, expired += 1;
            if (act && (cls == TETRA_TCH_FULL || cls == TETRA_TCH_HALF)) w.idle = 0, w.last = p;
            else if (act && cls == TETRA_TCH_CONTROL && fn != 18) {
                w.idle = d.idle + 1;
                if (w.idle > idle_max) w.active = 0, released += 1;
            }
        }
        __syncthreads();
    }
    while (more) {
        apply_event();
        next_event();
    }
    __syncthreads();
    if (lane < 4) {
        tetra_etsi_assign_slot *s = st->slot + lane;
        const Entry d = ent[lane];
        s->since = d.since;
        s->last = d.last;
        s->active = d.active;
        s->ssi = d.ssi;
        s->addr_type = d.addr_type;
        s->aux = d.aux;
        s->src_key = d.src_key;
        s->head = d.head;
        s->nalloc = d.nalloc;
        s->idle = d.idle;
    }
    if (lane == 0) {
        st->bit0 = bit0 + adv;
        st->expired = expired;
        st->released = released;
    }
}

}  // namespace

extern "C" int tetra_etsi_assign(tetra_ctx *ctx, const int32_t *nsym, size_t C, size_t G, int64_t row_bits, int64_t advance,
                                 int32_t hold_slots, int32_t idle_max, int32_t shared_clock, const int32_t *nburst,
                                 const int32_t *bursts, const int32_t *nblock, const int32_t *blocks, const int32_t *npdu,
                                 const int32_t *pdus, const int32_t *keep, const int32_t *slots, const int32_t *tq,
                                 const int32_t *sdu, int32_t maxd, const int32_t *ndone, const int32_t *done,
                                 const int32_t *row_key, tetra_etsi_assign_state *state, int32_t maxe, int32_t *nev,
                                 int32_t *ev, int32_t *ta) {
    if (!ctx) return TETRA_E_INVALID;
    const bool streaming = G == 1 && row_bits == 0 && !keep;
    if (C == 0 || !nburst || !bursts || !nblock || !blocks || !npdu || !pdus || !sdu || !ndone || !state || !nev || !ta ||
        (streaming && !nsym) || (maxd > 0 && !done) || (maxe > 0 && !ev))
        return tetra_fail(ctx, TETRA_E_INVALID,
                          "tetra_etsi_assign: C > 0 and every array but keep, slots, tq, row_key (nsym in the streaming form)");
    if (G < 1 || G > (size_t)MAXG || C % G != 0 || row_bits < 0 || maxe < 0 || maxd < 0 || hold_slots < 0 || idle_max < 0)
        return tetra_fail(ctx, TETRA_E_INVALID,
                          "tetra_etsi_assign: 1 <= G <= %d rows per group dividing C, row_bits, maxe, maxd, hold_slots and "
                          "idle_max >= 0 (C %zu, G %zu, row_bits %lld, maxe %d, maxd %d, hold_slots %d, idle_max %d)", MAXG, C,
                          G, (long long)row_bits, (int)maxe, (int)maxd, (int)hold_slots, (int)idle_max);
    if (C > ((size_t)1 << 24)) return tetra_fail(ctx, TETRA_E_INVALID, "too many rows for one tetra_etsi_assign call (%zu)", C);
    const size_t NG = C / G;
    // a group records at most min(maxe, its PDU records) events: the list's capacity
    const size_t cap = NG * std::min<size_t>((size_t)maxe, G * (size_t)MAXJ * MAXPDU);
    Staging st(ctx);
    // the int32 host arrays but the three largest travel as one staged input (four staged inputs in all)
    Staging::Part small[] = {{streaming ? nsym : nullptr, C}, {nburst, C}, {nblock, C}, {npdu, C * MAXJ}, {keep, C * MAXB},
                             {ndone, NG}, {row_key, NG}, {bursts, C * MAXB * 2}, {blocks, C * MAXJ * 4},
                             {slots, C * MAXB * NSL}, {tq, C * MAXB * NQ}};
    if (!st.pack(small)) return st.finish();
    const int32_t *ns = (const int32_t *)small[0].p, *nb = (const int32_t *)small[1].p, *nk = (const int32_t *)small[2].p,
                  *np = (const int32_t *)small[3].p, *kp = (const int32_t *)small[4].p, *ndn = (const int32_t *)small[5].p,
                  *rk = (const int32_t *)small[6].p, *bu = (const int32_t *)small[7].p, *bk = (const int32_t *)small[8].p,
                  *sl = (const int32_t *)small[9].p, *tqd = (const int32_t *)small[10].p;
    const int32_t *pd = (const int32_t *)st.in(pdus, C * MAXJ * MAXPDU * NF * 4);
    const int32_t *sd = (const int32_t *)st.in(sdu, C * MAXJ * MAXPDU * NS * 4);
    const int32_t *dn = maxd > 0 ? (const int32_t *)st.in(done, NG * (size_t)maxd * ND * 4) : nullptr;
    // in/out: what the kernels do not write keeps the caller's contents in host memory too
    tetra_etsi_assign_state *sa = (tetra_etsi_assign_state *)st.inout(state, NG * sizeof(tetra_etsi_assign_state));
    int32_t *ne = (int32_t *)st.out(nev, NG * 4);
    int32_t *eo = maxe > 0 ? (int32_t *)st.inout(ev, NG * (size_t)maxe * NE * 4) : nullptr;
    int32_t *to = (int32_t *)st.inout(ta, C * MAXB * NT * 4);
    int32_t *flag = (int32_t *)ws(ctx, S_W0, C * 4);
    // the list: the counter (16 bytes), the entries' times / sources / ordinals, their target keys
    char *lst = (char *)ws(ctx, S_W1, 16 + cap * (sizeof(Listed) + 4));
    if (!pd || !sd || (maxd > 0 && !dn) || !sa || !ne || (maxe > 0 && !eo) || !to || !flag || !lst) return st.finish();
    int32_t *count = (int32_t *)lst;
    Listed *clist = (Listed *)(lst + 16);
    int32_t *ckey = (int32_t *)(lst + 16 + cap * sizeof(Listed));
    {
        PROF(ctx, "etsi_assign");
        hipLaunchKernelGGL(k_assign_scan, dim3(grid_for(C * SCAN_LANES, SCAN_BLOCK)), dim3(SCAN_BLOCK), 0, ctx->stream, (int)C,
                           nb, nk, bk, np, pd, kp, sl, tqd, sd, flag, count, to);
        hipLaunchKernelGGL(k_assign_events, dim3((unsigned)NG), dim3(64), 0, ctx->stream, (int)G, row_bits, (int)maxe,
                           (int)maxd, (int)cap, nb, bu, nk, bk, np, pd, kp, sl, sd, ndn, dn, rk, flag, sa, ne, eo, count, ckey,
                           clist);
        hipLaunchKernelGGL(k_assign_follow, dim3((unsigned)NG), dim3(64), 0, ctx->stream, (int)G, row_bits, advance,
                           (int)hold_slots, (int)idle_max, (int)shared_clock, (int)maxe, (int)cap, ns, nb, bu, kp, sl, tqd, rk,
                           eo, count, ckey, clist, sa, to);
    }
    return st.finish();
}
