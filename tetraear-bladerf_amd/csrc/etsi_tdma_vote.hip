// etsi_tdma_vote.hip -- the timebase vote on gfx950 (tetra_etsi_mac_vote_groups): tetra_etsi_mac_groups
// with a SYNC weighed before it moves the slot grid, and each burst's best copy kept.  The walk of the
// blocks is etsi_mac.hip's k_mac_walk (etsi_mac.h); the weights are tetra_etsi_link_quality's records.
// The rule is in include/tetra_hip.h and, restated, in tests/_etsi_tdma_vote.py.
//
// The rule (exact integers, positions int64).
//   Order.  A group's live bursts (row i, b < nburst clamped to 0..MAXB) have pos = i row_bits + start
//     bit and are taken in the order (pos, row, b), as in tetra_etsi_mac_groups.
//   Clusters.  A cluster is a maximal run of that order in which every burst's pos exceeds the previous
//     burst's by at most tol_bits (the chain rule); its first burst is what tetra_etsi_mac_groups keeps.
//   Keep.  Burst (c, b) has a quality key Q.  good = the number of j < nblock[c] (clamped to 0..MAXJ)
//     with blocks[c][j] naming burst b, a kind in 0..2 and crc_ok != 0.  bq[c][b][TERR] < 0 (an invalid
//     burst): Q = -1.  Else Q = good << 32 | (60 - min(60, TERR + HERR)) << 16 | min(WSUM, 65535), with
//     TERR, HERR, WSUM from bq (a negative sum or WSUM, which no record has, reads as 0).  In every
//     cluster exactly one burst has keep = 1: the one with the largest Q, on a tie the first in the order.
//   Ballots.  A burst has an own SYNC as in tetra_etsi_mac_groups: an SB whose BSCH block is CRC-good
//     with a STATUS 0 record, of slot count s.  Its weight is w = max(1, WSUM - 2 WERR) from that block's
//     kq record, at most 15240 (a larger value, which no record has, reads as 15240); a kq record whose
//     NERR reads -1 gives w = 1.  In every cluster the own-SYNC burst with the largest w (on a tie the
//     first) is the cluster's ballot, cast where the walk reaches it; every other burst of the cluster is
//     walked as a burst without a SYNC.
//   The walk.  One per group over all live bursts in the order, kept or not, p = bit0 + pos.  State:
//     tdma[g] and score = max(0, tscore[g]).  Rule 1 of tetra_etsi_mac_groups gives (pred, k); a lock
//     that expires (k >= TETRA_TDMA_EXPIRE) also sets score to 0.  For a ballot (s, w):
//       a. not locked: anchor = (p, s), locked, score = min(cap, w); the row is s, FLAGS 1; BALLOTS++;
//       b. locked and pred == s: score = min(cap, score + w), anchor = (p, s); the row is s, FLAGS 1;
//          BALLOTS++, AGREED++;
//       c. locked and pred != s (another slot, or none): if w > score the ballot wins: anchor = (p, s),
//          score = min(cap, w - score); the row is s, FLAGS 1 | 2; BALLOTS++, WON++.  Otherwise score -=
//          w; if pred is a slot the burst takes it with FLAGS 2 | 4 (bit 2: own SYNC outvoted) and the
//          anchor moves to (p, pred) only if k >= 1; if pred is none the row reads 0, 0, 0, 0;
//          BALLOTS++, OUTVOTED++.
//     Every other burst follows rules 3 and 4 of tetra_etsi_mac_groups.  After the walk bit0 += advance
//     and tscore[g] = score; without a ballot tscore changes only by expiry (and a negative one to 0).
//
//   k_tdma_vote_groups  one wave per group, at most 8 G = 512 entries in LDS, k_tdma_groups's rank sort on
//               (pos, e).  Lane e % 64 prepares entry e (pos, own-SYNC slot, w, Q); after the sort a lane
//               marks the cluster heads among its ranks from the neighbour in the order, and the lane of
//               a head walks its cluster for the two arg-max results (Q for keep, w for the ballot);
//               lane 0 then walks the order.  Every data-dependent index is an LDS address.
#include "etsi_mac.h"

namespace {

constexpr int MAXB = TETRA_ETSI_MAXB, MAXJ = TETRA_ETSI_MAXJ, MAXPDU = TETRA_ETSI_MAXPDU, NF = TETRA_PDU_FIELDS;
constexpr int NQ = TETRA_LQ_FIELDS;
constexpr int MAXG = 64, MAXE = MAXG * MAXB;   // rows per group, burst entries per group
constexpr int64_t K_SPAN = 510 * (int64_t)TETRA_TDMA_EXPIRE - 255;   // d >= K_SPAN: k >= EXPIRE; d < -K_SPAN: k <= -EXPIRE
constexpr int W_MAX = 120 * 127;               // a BSCH block's largest WSUM
static_assert(TETRA_TV_FIELDS == 4 && TETRA_SLOT_FIELDS == 4 && MAXE <= 65536, "record layout");

// One wave per group.  Entry e = row * MAXB + b, so the order (pos, row, b) is (pos, e).
__global__ __launch_bounds__(64) void k_tdma_vote_groups(
    int G, int64_t row_bits, int64_t tol_bits, int64_t advance, int cap, const int32_t *__restrict__ nburst,
    const int32_t *__restrict__ bursts, const int32_t *__restrict__ nblock, const int32_t *__restrict__ blocks,
    const int32_t *__restrict__ own, const int32_t *__restrict__ bq, const int32_t *__restrict__ kq,
    tetra_etsi_tdma *tdma, int32_t *tscore, int32_t *__restrict__ keep, int32_t *__restrict__ slots,
    int32_t *__restrict__ tvote) {
    __shared__ int64_t pos[MAXE];
    __shared__ int64_t qkey[MAXE];    // Q
    __shared__ int32_t ownv[MAXE];    // own-SYNC slot count, -1 none, DEAD past the row's nburst
    __shared__ int32_t wgt[MAXE];     // w of an own-SYNC entry
    __shared__ int32_t res[MAXE];     // by entry: slot | flags << 16, -1 unknown
    __shared__ int32_t bal[MAXE];     // by rank: the slot count of the ballot cast there, -1 none
    __shared__ uint16_t order[MAXE];  // rank -> entry
    __shared__ uint8_t head[MAXE];    // by rank: the first of its cluster
    constexpr int32_t DEAD = INT32_MIN;
    const int lane = threadIdx.x, ne = G * MAXB;
    const size_t c0 = (size_t)blockIdx.x * G;
    int mine = 0;
    for (int e = lane; e < ne; e += 64) {
        const int i = e / MAXB, b = e % MAXB;
        const size_t c = c0 + i;
        const bool live = b < min(max(nburst[c], 0), MAXB);
        int64_t p = 0, q = -1;
        int32_t o = DEAD, w = 1;
        if (live) {
            const int32_t *bu = bursts + c * MAXB * 2;
            p = (int64_t)((uint64_t)i * (uint64_t)row_bits) + bu[2 * b];
            o = own[c * MAXB + b];
            if (o >= 0) {   // the BSCH block of burst b by the sync kernel's numbering (below MAXJ: k_mac_walk)
                int j = 0;
                for (int a = 0; a < b; ++a) j += bu[2 * a + 1] == TETRA_NDB_N ? 1 : 2;
                const int32_t *k = kq + (c * MAXJ + min(j, MAXJ - 1)) * NQ;
                if (k[TETRA_LQ_NERR] >= 0) {
                    const int64_t d = (int64_t)k[TETRA_LQ_WSUM] - 2 * (int64_t)k[TETRA_LQ_WERR];
                    w = (int32_t)(d < 1 ? 1 : d > W_MAX ? W_MAX : d);
                }
            }
            const int32_t *r = bq + (c * MAXB + b) * NQ;
            if (r[TETRA_BQ_TERR] >= 0) {
                const int nk = min(max(nblock[c], 0), MAXJ);
                int good = 0;
                for (int j = 0; j < nk; ++j) {
                    const int32_t *bk = blocks + (c * MAXJ + j) * 4;
                    good += (int)(bk[2] == b) & (int)(bk[0] >= 0) & (int)(bk[0] <= 2) & (int)(bk[1] != 0);
                }
                const int64_t t = (int64_t)r[TETRA_BQ_TERR] + r[TETRA_BQ_HERR];
                const int err = (int)(t < 0 ? 0 : t > 60 ? 60 : t);
                q = (int64_t)good << 32 | (int64_t)(60 - err) << 16 | min(max(r[TETRA_BQ_WSUM], 0), 65535);
            }
        }
        pos[e] = p;
        qkey[e] = q;
        ownv[e] = o;
        wgt[e] = w;
        mine += live;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m, 64);
    const int n = mine;   // the group's live bursts
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
    for (int r = lane; r < n; r += 64)   // the chain rule: against the previous in order
        head[r] = r == 0 || pos[order[r]] - pos[order[r - 1]] > tol_bits;
    __syncthreads();
    for (int r = lane; r < n; r += 64) {   // a head's lane walks its cluster: ranks r .. the next head
        if (!head[r]) continue;
        int rq = r, rw = -1, end = r;
        int64_t bestq = INT64_MIN;
        int32_t bestw = 0;
        do {
            const int e = order[end];
            const int64_t q = qkey[e];
            if (q > bestq) {
                bestq = q;
                rq = end;
            }
            if (ownv[e] >= 0 && wgt[e] > bestw) {   // w >= 1
                bestw = wgt[e];
                rw = end;
            }
            ++end;
        } while (end < n && !head[end]);
        for (int t = r; t < end; ++t) {
            const int e = order[t];
            keep[(c0 + e / MAXB) * MAXB + e % MAXB] = t == rq;
            bal[t] = t == rw ? ownv[e] : -1;
        }
    }
    __syncthreads();
    if (lane == 0) {
        tetra_etsi_tdma *td = tdma + blockIdx.x;
        const int64_t bit0 = td->bit0;
        int64_t abit = td->anchor_bit;
        int aslot = td->anchor_slot;
        bool locked = td->locked != 0;
        int score = max(tscore[blockIdx.x], 0);
        int nbal = 0, nagree = 0, nout = 0, nwon = 0;
        for (int r = 0; r < n; ++r) {
            const int e = order[r];
            const int64_t p = bit0 + pos[e];
            int pred = -1, k = 0;
            if (locked) {
                const int64_t d = p - abit;
                if (d >= K_SPAN) {
                    locked = false;
                    score = 0;
                } else if (d >= -K_SPAN) {
                    const int x = (int)d + 255;
                    k = x >= 0 ? x / 510 : -((509 - x) / 510);
                    const int rr = (int)d - 510 * k;
                    if (rr >= -TETRA_TDMA_TOL && rr <= TETRA_TDMA_TOL)
                        pred = (aslot + k + TETRA_TDMA_SLOTS) % TETRA_TDMA_SLOTS;
                }
            }
            const int s = bal[r];
            int out = pred;
            bool move = pred >= 0 && k >= 1;   // rule 3 of tetra_etsi_mac_groups; an outvoted ballot likewise
            int to = pred;
            if (s >= 0) {
                const int w = wgt[e];
                ++nbal;
                if (!locked || pred == s || w > score) {   // a, b, or c won
                    const int64_t sc = !locked ? w : pred == s ? (int64_t)score + w : (int64_t)w - score;
                    const bool won = locked && pred != s;
                    nagree += locked && pred == s;
                    nwon += won;
                    score = (int)min(sc, (int64_t)cap);
                    out = s | (won ? 3 : 1) << 16;
                    locked = true;
                    move = true;
                    to = s;
                } else {   // c outvoted
                    score -= w;
                    ++nout;
                    if (pred >= 0) out = pred | 6 << 16;
                }
            }
            if (move) {
                abit = p;
                aslot = to;
            }
            res[e] = out;
        }
        td->bit0 = bit0 + advance;
        td->anchor_bit = abit;
        td->anchor_slot = aslot;
        td->locked = locked;
        tscore[blockIdx.x] = score;
        int32_t *tv = tvote + (size_t)blockIdx.x * TETRA_TV_FIELDS;
        tv[TETRA_TV_BALLOTS] = nbal;
        tv[TETRA_TV_AGREED] = nagree;
        tv[TETRA_TV_OUTVOTED] = nout;
        tv[TETRA_TV_WON] = nwon;
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

extern "C" int tetra_etsi_mac_vote_groups(tetra_ctx *ctx, const int32_t *nsym, size_t C, size_t G, int64_t row_bits,
                                          int64_t tol_bits, int64_t advance, int32_t cap, const int32_t *nburst,
                                          const int32_t *bursts, const int32_t *nblock, const int32_t *blocks,
                                          const uint8_t *type1, const int32_t *bq, const int32_t *kq,
                                          tetra_etsi_tdma *tdma, int32_t *tscore, int32_t *keep, int32_t *slots,
                                          int32_t *npdu, int32_t *pdus, int32_t *tvote) {
    if (!ctx) return TETRA_E_INVALID;
    if (C == 0 || !nsym || !nburst || !bursts || !nblock || !blocks || !type1 || !bq || !kq || !tdma || !tscore || !keep ||
        !slots || !npdu || !pdus || !tvote)
        return tetra_fail(ctx, TETRA_E_INVALID, "tetra_etsi_mac_vote_groups: C > 0 and every array");
    if (G < 1 || G > (size_t)MAXG || C % G != 0 || row_bits < 0 || tol_bits < 0 || cap <= 0)
        return tetra_fail(ctx, TETRA_E_INVALID,
                          "tetra_etsi_mac_vote_groups: 1 <= G <= %d rows per group dividing C, row_bits and tol_bits >= 0, "
                          "cap > 0 (C %zu, G %zu, row_bits %lld, tol_bits %lld, cap %d)", MAXG, C, G, (long long)row_bits,
                          (long long)tol_bits, (int)cap);
    if (C > ((size_t)1 << 24))
        return tetra_fail(ctx, TETRA_E_INVALID, "too many rows for one tetra_etsi_mac_vote_groups call (%zu)", C);
    const size_t NG = C / G;
    Staging st(ctx);
    // the two count arrays travel as one staged input (six staged inputs at most)
    Staging::Part small[] = {{nburst, C}, {nblock, C}};
    if (!st.pack(small)) return st.finish();
    const int32_t *nb = (const int32_t *)small[0].p, *nk = (const int32_t *)small[1].p;
    const int32_t *bu = (const int32_t *)st.in(bursts, C * MAXB * 2 * 4);
    const int32_t *bk = (const int32_t *)st.in(blocks, C * MAXJ * 4 * 4);
    const uint8_t *t1 = (const uint8_t *)st.in(type1, C * MAXJ * 268);
    const int32_t *bqd = (const int32_t *)st.in(bq, C * MAXB * NQ * 4);
    const int32_t *kqd = (const int32_t *)st.in(kq, C * MAXJ * NQ * 4);
    tetra_etsi_tdma *td = (tetra_etsi_tdma *)st.inout(tdma, NG * sizeof(tetra_etsi_tdma));
    int32_t *ts = (int32_t *)st.inout(tscore, NG * 4);
    // in/out: what the kernels do not write keeps the caller's contents in host memory too
    int32_t *kp = (int32_t *)st.inout(keep, C * MAXB * 4);
    int32_t *so = (int32_t *)st.inout(slots, C * MAXB * TETRA_SLOT_FIELDS * 4);
    int32_t *np = (int32_t *)st.out(npdu, C * MAXJ * 4);
    int32_t *po = (int32_t *)st.inout(pdus, C * MAXJ * MAXPDU * NF * 4);
    int32_t *tv = (int32_t *)st.out(tvote, NG * TETRA_TV_FIELDS * 4);
    int32_t *own = (int32_t *)ws(ctx, S_W0, C * MAXB * 4);
    if (!nb || !nk || !bu || !bk || !t1 || !bqd || !kqd || !td || !ts || !kp || !so || !np || !po || !tv || !own)
        return st.finish();
    {
        PROF(ctx, "etsi_mac_vote_groups");
        launch_mac_walk(ctx, C, nb, bu, nk, bk, t1, own, np, po);
        hipLaunchKernelGGL(k_tdma_vote_groups, dim3((unsigned)NG), dim3(64), 0, ctx->stream, (int)G, row_bits, tol_bits,
                           advance, (int)cap, nb, bu, nk, bk, own, bqd, kqd, td, ts, kp, so, tv);
    }
    return st.finish();
}
