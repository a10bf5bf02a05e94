// etsi_lmac.hip -- ETSI EN 300 392-2 lower MAC on gfx950: burst sync and channel decoding of the
// rows the ETSI timing stage (etsi_timing.h) writes (hard dibits, int8 soft bits, nsym), the second half
// of the north-star receive chain, restating oracle/etsi_oracle.c bit for bit.
//
//   k_etsi_sync  one wave per channel: hard bits packed by ballots, head/training/tail correlation
//                by XOR+popcount, greedy burst scan, one decode job per coded block (dense atomic
//                allocation).
//   k_etsi_viterbi  four lanes per job: the block's type-5 soft bits loaded as dwords and
//                descrambled into an LDS row, deinterleave + depuncture applied on the trellis's
//                reads, 16-state rate-1/4 Viterbi with metrics in registers, survivors coalesced in
//                global scratch.
//   k_etsi_traceback  one lane per job: traceback with the CRC-16 folded in.
//   k_etsi_tail  streaming: a channel's undecoded tail moved to the front of the next chunk's rows.
//   k_cell_acquire  one lane per channel: the scrambling init from the chunk's last CRC-good BSCH.
//   k_cell_acquire_groups  one wave per group of rows (a carrier's chunks): the same rule over the
//                group's rows in order, the scrambler sequence formed once and stored to its rows.
//   k_decode_blocks, k_encode_blocks  the channel coding of independent blocks of one kind
//                (component entry points: tetra_etsi_decode_blocks / _encode_blocks).
#include <cstdlib>

#include "common.h"
#include "etsi_coding.h"   // block kinds, burst patterns, puncturer, CRC and scrambler tables
#include "etsi_vote.h"     // the cell vote's launch (etsi_vote.hip)

namespace {

// --------------------------------------------------------------------------- E3/E4 lower MAC
// up to 32 stream bits from pos, from the 32-bit view of the words: one funnel shift
__device__ __forceinline__ uint32_t bits32_at(const uint32_t *w, int pos) {
    const int q = pos >> 5;
    return __builtin_amdgcn_alignbit(w[q + 1], w[q], (uint32_t)(pos & 31));
}
__device__ __forceinline__ int matches32(uint32_t v, uint32_t pat, int len) {
    return len - __popc((v ^ pat) & (len == 32 ? 0xFFFFFFFFu : ((1u << len) - 1)));
}

constexpr int LMAC_MAXBITS = 2 * 2048;

// --------------------------------------------------------------------------- E3 burst sync
struct Job {
    int ch, slot, burst, blk, kind, off;
};

// Job regions, one per block kind, so every Viterbi wave runs a single trellis length:
// SCH/F [0, 8C), SCH/HD [8C, 24C), BSCH [24C, 32C) (<= 8 bursts per channel chunk).
__host__ __device__ inline size_t job_base(int kind, size_t C) { return kind == 0 ? 0 : kind == 1 ? 8 * C : 24 * C; }
__host__ __device__ inline size_t job_cap(int kind, size_t C) { return kind == 1 ? 16 * C : 8 * C; }

// One wave per channel: pack hard bits, greedy burst scan, then allocate this channel's coded
// blocks dense job indices in each kind's region (one atomic per kind per channel; outputs are
// indexed by (channel, slot), so results do not depend on the allocation order).
constexpr int SYNC_WAVES = 4;   // channels per workgroup: one job-counter atomic per workgroup

struct SyncLds {
    uint64_t words_all[SYNC_WAVES][LMAC_MAXBITS / 64 + 2];
    int bstart_all[SYNC_WAVES][ETSI_MAXB], bkind_all[SYNC_WAVES][ETSI_MAXB];
    int per_all[SYNC_WAVES][3];
    unsigned long long block_old;
};

// Streaming: the dibits (and their soft bits) the scan left unconsumed -- from row dibit td0, T of
// them -- go in front of column R of the next rows, and lead[c] to their first unexamined bit (one
// wave).  Into other rows straight from k_etsi_sync; into these rows (tinfo) by k_etsi_tail, after
// the trellis has read them.
__device__ __forceinline__ void tail_move(const uint8_t *hard, const int8_t *soft, int stride, int ch, int td0, int T,
                                          int ph, int R, uint8_t *nhard, int8_t *nsoft, int32_t *lead, int lane) {
    const uint8_t *hrow = hard + (size_t)ch * stride;
    const int8_t *srow = soft + (size_t)ch * 2 * stride;
    uint8_t hv[4];
    int8_t s0[4], s1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = lane + 64 * u;
        hv[u] = i < T ? hrow[td0 + i] : 0;
        s0[u] = i < T ? srow[2 * (td0 + i)] : 0;
        s1[u] = i < T ? srow[2 * (td0 + i) + 1] : 0;
    }
    __builtin_amdgcn_s_waitcnt(0);   // every read done before a write (the rows may be these rows)
    __builtin_amdgcn_wave_barrier();
    uint8_t *nh = nhard + (size_t)ch * stride;
    int8_t *ns = nsoft + (size_t)ch * 2 * stride;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = lane + 64 * u;
        if (i < T) {
            nh[R - T + i] = hv[u];
            ns[2 * (R - T + i)] = s0[u];
            ns[2 * (R - T + i) + 1] = s1[u];
        }
    }
    if (lane == 0) lead[ch] = 2 * (R - T) + ph;
}

// Streaming (lead != null, tetra_lmac_etsi_stream): row c holds the previous chunk's unconsumed
// dibits in front of column R and this chunk's from R; the scan starts at row bit lead[c] and
// afterwards the dibits from the first bit not examined move in front of column R of the next rows
// (nsoft / nhard), lead[c] pointing at their first bit -- oracle/etsi.py Stream.
__device__ __forceinline__ void sync_group(SyncLds &L, int grp, const uint8_t *__restrict__ hard,
                                           const int32_t *__restrict__ nsym, int smax, int32_t *__restrict__ nburst,
                                           int32_t *__restrict__ bursts, int32_t *__restrict__ nblock,
                                           unsigned long long *__restrict__ jcount, Job *__restrict__ jobs, int C,
                                           int32_t *lead, int R, int32_t *tinfo, const int8_t *soft, uint8_t *nhard,
                                           int8_t *nsoft) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ch = grp * SYNC_WAVES + wv;
    auto &words_all = L.words_all;
    auto &bstart_all = L.bstart_all;
    auto &bkind_all = L.bkind_all;
    auto &per_all = L.per_all;
    auto &block_old = L.block_old;
    uint64_t *words = words_all[wv];
    int *bstart = bstart_all[wv], *bkind = bkind_all[wv];
    const int S = ch < C ? nsym[ch] : 0;
    const int nd = S > 1 ? S - 1 : 0;
    int d0 = 0, cur0 = 0, nrow = nd;   // the scan's first dibit / bit, the row's dibits from d0
    if (lead) {
        const int b = ch < C ? min(max(lead[ch], 0), 2 * R) : 2 * R;
        d0 = b >> 1;
        cur0 = b & 1;
        nrow = R + nd - d0;
    }
    // every bit of the widest row the host admits (2 smax <= LMAC_MAXBITS + 4): words_all holds
    // LMAC_MAXBITS + 128 bits, the last extraction (s + 500, 32 bits on) ends 22 bits past the scan's
    int nbits = 2 * nrow;
    if (nbits > LMAC_MAXBITS + 4) nbits = LMAC_MAXBITS + 4;
    const uint8_t *hp = hard + (size_t)ch * smax + d0;
    const int lim = smax - d0;   // the row's symbols from hp
    // pack hard bits with ballots: a word holds 32 dibit symbols (bit 2i = b1, 2i+1 = b2), so lane j
    // of the ballot contributes bit j of the word: component j & 1 of symbol j >> 1.  Two ballots per
    // 64 symbols and no bit interleave (interleaving two 32-bit ballots was ~80 scalar 64-bit ops per
    // word, on the CU's one scalar unit shared by all its waves)
    const int nsy = nbits / 2;
    // symbols loaded 8 steps (512 symbols) at a time, all before the first ballot: a load per step
    // in the dependent loop cost one memory latency per 64 symbols
    constexpr int PK = 8;
    const int sl = lane >> 1, comp = lane & 1;
    for (int s00 = 0; s00 < nsy + 64; s00 += 64 * PK) {
    uint32_t hA[PK], hB[PK];
#pragma unroll
    for (int u = 0; u < PK; ++u) {
        const int s = s00 + 64 * u + sl;
        hA[u] = hp[min(s, lim - 1)];   // unconditional (in the row): no branch join waits per load
        hB[u] = hp[min(s + 32, lim - 1)];
    }
#pragma unroll
    for (int u = 0; u < PK; ++u) {
        const int s0 = s00 + 64 * u;
        if (s0 >= nsy + 64) break;   // uniform
        const int s = s0 + sl;
        const uint32_t a = s < nsy ? (comp ? hA[u] : hA[u] >> 1) & 1u : 0u;
        const uint32_t b = s + 32 < nsy ? (comp ? hB[u] : hB[u] >> 1) & 1u : 0u;
        const uint64_t wa = __ballot(a), wb = __ballot(b);
        if (lane == 0 && s0 / 32 + 1 < LMAC_MAXBITS / 64 + 2) {
            words[s0 / 32] = wa;
            words[s0 / 32 + 1] = wb;
        }
    }
    }
    __syncthreads();
    int nb = 0;
    int nextpos = cur0;   // the first position not examined (streaming: where the next chunk resumes)
    for (int cur = cur0; cur + 510 <= nbits && nb < ETSI_MAXB;) {
        const int s = cur + lane;
        int kind = -1;
        if (s + 510 <= nbits) {
            // 32-bit funnel-shift extractions (words viewed as little-endian dwords: stream bit p is
            // bit p & 31 of dword p >> 5)
            const uint32_t *w32 = reinterpret_cast<const uint32_t *>(words);
            const int ht = matches32(bits32_at(w32, s), (uint32_t)W_HEAD, 12) +
                           matches32(bits32_at(w32, s + 500), (uint32_t)W_TAIL, 10);
            const uint32_t t22 = bits32_at(w32, s + 244);
            const int mn = ht + matches32(t22, (uint32_t)W_N, 22), mp = ht + matches32(t22, (uint32_t)W_P, 22);
            const int my = ht + matches32(bits32_at(w32, s + 214), (uint32_t)W_Y, 32) +
                           matches32(bits32_at(w32, s + 246), (uint32_t)(W_Y >> 32), 6);
            if (my >= 54) kind = 2;
            else if (mn >= 40 && mn >= mp) kind = 0;
            else if (mp >= 40) kind = 1;
        }
        const unsigned long long bal = __ballot(kind >= 0);
        if (bal) {
            const int first = __ffsll((long long)bal) - 1;
            const int k = __builtin_amdgcn_readlane(kind, first);   // first is wave-uniform
            if (lane == 0) { bstart[nb] = cur + first; bkind[nb] = k; }
            ++nb;
            cur = cur + first + 500;
            nextpos = cur;
        } else {
            cur += 64;
            nextpos = min(cur, nbits - 509);
        }
    }
    if (lead && ch < C) {   // the unconsumed tail
        int td0 = d0 + (nextpos >> 1), ph = nextpos & 1;
        int T = R + nd - td0;
        if (T > R) { td0 = nd; T = R; ph = 0; }   // (past ETSI_MAXB bursts only) keep the last R dibits
        if (T < 0) { td0 = R + nd; T = 0; ph = 0; }
        if (nhard) {   // other rows (double-buffered): moved here, the trellis reads only these rows
            tail_move(hard, soft, smax, ch, td0, T, ph, R, nhard, nsoft, lead, lane);
        } else if (lane == 0) {   // these rows: k_etsi_tail moves it after the trellis has read them
            tinfo[2 * ch] = td0;
            tinfo[2 * ch + 1] = (T << 1) | ph;
        }
    }
    __syncthreads();
    int per[3] = {0, 0, 0};
    if (lane == 0) {   // blocks per kind: normal-n 1 SCH/F; normal-p 2 SCH/HD; sync BSCH + SCH/HD
        for (int b = 0; b < nb; ++b) {
            if (bkind[b] == 0) ++per[0];
            else if (bkind[b] == 1) per[1] += 2;
            else { ++per[2]; ++per[1]; }
        }
        for (int k = 0; k < 3; ++k) per_all[wv][k] = per[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {   // the workgroup's three kind counters, packed 21 bits apart: one atomic
        unsigned long long inc = 0;
        for (int w = 0; w < SYNC_WAVES; ++w)
            inc += (unsigned long long)per_all[w][0] | ((unsigned long long)per_all[w][1] << 21) |
                   ((unsigned long long)per_all[w][2] << 42);
        block_old = inc ? atomicAdd(jcount, inc) : 0ull;
    }
    __syncthreads();
    if (lane == 0 && ch < C) {
        nburst[ch] = nb;
        nblock[ch] = per[0] + per[1] + per[2];
        int next[3];
        for (int k = 0; k < 3; ++k) {
            next[k] = (int)job_base(k, C) + (int)((block_old >> (21 * k)) & 0x1FFFFFull);
            for (int w = 0; w < wv; ++w) next[k] += per_all[w][k];
        }
        int q = 0;
        for (int b = 0; b < nb; ++b) {
            const int s = 2 * d0 + bstart[b], k = bkind[b];   // row bit (= the soft-bit row index)
            bursts[((size_t)ch * ETSI_MAXB + b) * 2] = s - 2 * R * (lead != nullptr);   // from the chunk's first new dibit
            bursts[((size_t)ch * ETSI_MAXB + b) * 2 + 1] = k;
            if (k == 0) {
                jobs[next[0]++] = Job{ch, q, b, 0, 0, s + 14}; ++q;
            } else if (k == 1) {
                jobs[next[1]++] = Job{ch, q, b, 0, 1, s + 14}; ++q;
                jobs[next[1]++] = Job{ch, q, b, 1, 1, s + 282}; ++q;
            } else {
                jobs[next[2]++] = Job{ch, q, b, 0, 2, s + 94}; ++q;
                jobs[next[1]++] = Job{ch, q, b, 1, 1, s + 282}; ++q;
            }
        }
    }
}


// Grid: one workgroup per SYNC_WAVES channels (the loop is a grid stride).
__global__ __launch_bounds__(64 * SYNC_WAVES) void k_etsi_sync(const uint8_t *__restrict__ hard, const int32_t *__restrict__ nsym,
                                                  int smax, int32_t *__restrict__ nburst, int32_t *__restrict__ bursts,
                                                  int32_t *__restrict__ nblock,
                                                  unsigned long long *__restrict__ jcount, Job *__restrict__ jobs,
                                                  int C, int32_t *lead, int R, int32_t *tinfo, const int8_t *soft,
                                                  uint8_t *nhard, int8_t *nsoft) {
    __shared__ SyncLds L;
    const int ng = (C + SYNC_WAVES - 1) / SYNC_WAVES;
    for (int g = blockIdx.x; g < ng; g += gridDim.x) {
        sync_group(L, g, hard, nsym, smax, nburst, bursts, nblock, jcount, jobs, C, lead, R, tinfo, soft, nhard,
                   nsoft);
        __syncthreads();   // L is reused by the next group
    }
}

__global__ __launch_bounds__(64) void k_etsi_tail(const uint8_t *__restrict__ hard, const int8_t *__restrict__ soft,
                                                  int stride, int C, const int32_t *__restrict__ tinfo, int R,
                                                  uint8_t *nhard, int8_t *nsoft, int32_t *__restrict__ lead) {
    const int ch = blockIdx.x;
    if (ch >= C) return;
    tail_move(hard, soft, stride, ch, tinfo[2 * ch], tinfo[2 * ch + 1] >> 1, tinfo[2 * ch + 1] & 1, R, nhard, nsoft,
              lead, threadIdx.x);
}

// --------------------------------------------------------------------------- E4 Viterbi
// Four LANES per coded block (one DPP quad) holding the 16 path metrics (layout below).  The quad loads
// the block's type-5 soft bits into one shared LDS row, descrambled (load_seg: 16 contiguous bytes
// per quad per load; the byte gather this replaced -- two scattered byte loads per soft bit -- was
// what the Viterbi cost the demod running beside it), and the trellis reads that row through the
// deinterleaver (acs_groups4); each lane packs its 4 decision bits of 8
// steps into one survivor dword ([group][job][lane], coalesced); all four lanes trace back (same
// path) and lane 0 writes the block with the CRC accumulated on the fly.  16 blocks per 64-lane
// workgroup keep LDS at 7 KB, so Viterbi workgroups fit beside the demod's on a CU.
constexpr int VROW = 436;   // LDS row per block: 432 type-3 values, padded to 109 dwords (bank spread)

template <int CTRL>
__device__ __forceinline__ int32_t quad_perm(int32_t v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}

// One contiguous segment of a block's type-5 soft bits (ND dwords) into the LDS row, descrambled.
// The quad reads the segment as aligned dwords, lane q taking dwords 4 i + q (16 contiguous bytes
// per quad per load), and realigns them with v_alignbyte, the next dword coming from the neighbour
// lane (quad rotate) or, for lane 3, from lane 0 of the next load.  A dword is loaded only if it
// starts at or before the buffer's last byte (`last`, a dword that holds it): a clamped load reads
// bytes the segment does not use.  Descrambling negates the int8 values whose scrambler byte is 1
// (four at a time: x ^ 0xFF + 1 per flagged byte, carry-free SWAR), as -v in int8 does.
// The loads go through buffer resources over the whole soft-bit buffer (sbr: from the dword that
// holds its first byte to the dword that holds its last) and the scrambler table (scr_r): one 32-bit
// offset per lane with the load index in the immediate field, where 64-bit clamped addresses held two
// VGPRs per load in flight; a load past the buffer returns 0 instead of the clamped dword (bytes the
// segment does not use either way).  seg_off: the segment's byte offset from sbr's base (whose
// alignment is the buffer's: sbr starts at a dword boundary), scr_off: the table segment's.
template <int ND>
__device__ __forceinline__ void load_seg(__amdgpu_buffer_rsrc_t sbr, uint32_t seg_off, __amdgpu_buffer_rsrc_t scr_r,
                                         uint32_t scr_off, uint32_t *d32, int q) {
    constexpr int NI = (ND + 1 + 3) / 4;   // loads per lane: dwords 0 .. ND of the aligned window
    const int sh = (int)(seg_off & 3);
    const uint32_t a0 = seg_off - sh + 4 * q, s0 = scr_off + 4 * q;
    uint32_t R[NI], S[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        R[i] = __builtin_amdgcn_raw_buffer_load_b32(sbr, a0 + 16 * i, 0, 0);
        S[i] = __builtin_amdgcn_raw_buffer_load_b32(scr_r, s0 + 16 * i, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = 4 * i + q;
        const uint32_t nq = (uint32_t)quad_perm<0x39>((int32_t)R[i]);   // lane (q + 1) & 3
        const uint32_t n0 = i + 1 < NI ? (uint32_t)quad_perm<0x00>((int32_t)R[i + 1]) : 0u;
        const uint32_t v = __builtin_amdgcn_alignbyte(q == 3 ? n0 : nq, R[i], (uint32_t)sh);
        const uint32_t m = S[i] * 0xFFu, x = v ^ m;   // scrambler bytes are 0 / 1
        const uint32_t dv = ((x & 0x7F7F7F7Fu) + (m & 0x01010101u)) ^ (x & 0x80808080u);
        if (j < ND) d32[j] = dv;
    }
}

// Strided state layout: lane l of the quad holds states n = 4 i + l in pm[i].  New state n has
// predecessors p0 = n >> 1 = 2 i + (l >> 1) (register i >> 1 of lane (2 i + (l >> 1)) & 3) and
// p1 = p0 | 8 (register (i >> 1) + 2, same lane): for a given i both sit in one register of a lane
// that one quad_perm pattern names, so each new metric takes two DPP moves and no selects.  The
// branch-metric signs depend on n & 3 = l (lane constants) and on n >> 2 = i (compile time).
// Survivors: a lane packs its 4 decision bits of 8 consecutive steps into one dword (bit
// 4 (t & 7) + i for state 4 i + l at step t) and stores it once per 8 steps, [group][job][lane]:
// one coalesced 256-B store per wave per 8 steps.
// The row holds the descrambled block in type-5 order; the deinterleaver is applied on the read:
// type-3 value i (1-based) is type-5 value k(i) = 1 + (A i mod K).  The index walk is the same for
// every lane of the wave (one block kind per wave), so it stays in scalar registers.
template <int GROUPS, int A, int K>
__device__ __forceinline__ void acs_groups4(int32_t (&pm)[4], int q, const int8_t *row, uint32_t *sv, size_t gstride) {
    // rate-2/3 puncturing: step 2g sees mother outputs (g1, g2) = type-3 (3g, 3g+1); step 2g+1 sees
    // g1 = type-3 3g+2; the other mother outputs are erased.
    const bool bb = q & 1, d0 = (q >> 1) & 1;   // bits 0 and 1 of this lane's states
    int r = 0;   // A i mod K for the type-3 value read last
    auto next = [&r]() {
        r += A;
        if (r >= K) r -= K;
        return r;
    };
    for (int gi = 0; gi < GROUPS; ++gi) {
        uint32_t word = 0;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int i0 = next(), i1 = next(), i2 = next();
            const int32_t a = row[i0], b = row[i1], c = row[i2];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                // branch metric for d3 = 0 (d3 = 1 negates every generator output):
                // step 2g: +-a +-b (b's sign also flips with (n >> 2) ^ (n >> 3)); step 2g+1: +-c
                int32_t v0, v1;
                if (half == 0) {
                    const int32_t sa = (bb ^ d0) ? -a : a, sb = bb ? -b : b;
                    v0 = sa + sb;   // i with flip 0 (i = 0, 3)
                    v1 = sa - sb;   // flip 1 (i = 1, 2)
                } else {
                    v0 = v1 = (bb ^ d0) ? -c : c;
                }
                const int32_t X0 = quad_perm<0x50>(pm[0]), Y0 = quad_perm<0x50>(pm[2]);
                const int32_t X1 = quad_perm<0xFA>(pm[0]), Y1 = quad_perm<0xFA>(pm[2]);
                const int32_t X2 = quad_perm<0x50>(pm[1]), Y2 = quad_perm<0x50>(pm[3]);
                const int32_t X3 = quad_perm<0xFA>(pm[1]), Y3 = quad_perm<0xFA>(pm[3]);
                const int32_t X[4] = {X0, X1, X2, X3}, Y[4] = {Y0, Y1, Y2, Y3};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int32_t v = ((i ^ (i >> 1)) & 1) ? v1 : v0;
                    const int32_t m0 = X[i] + v, m1 = Y[i] - v;
                    const bool t1 = m1 > m0;
                    pm[i] = t1 ? m1 : m0;
                    word |= (uint32_t)t1 << (4 * (2 * g4 + half) + i);
                }
            }
        }
        sv[(size_t)gi * gstride] = word;
    }
}

// soft-bit and scrambler-table resources of one k_etsi_viterbi launch (wave-uniform)
struct VitSrc {
    __amdgpu_buffer_rsrc_t sbr, cell_r, bsch_r;
    uint32_t sb_lead;   // bytes from sbr's base (a dword boundary) to softbits[0]
};

template <int KIND>
__device__ __forceinline__ void viterbi_wave(int8_t *rows, const Job *__restrict__ jobs, int nj, size_t jbase, int lb,
                                             size_t ss, const VitSrc &src, int smax, uint32_t *__restrict__ surv) {
    constexpr KindP P = kind_params(KIND);
    const int lane = threadIdx.x, jw = lane >> 2, q = lane & 3;
    const int jl = lb * 16 + jw;
    if (lb * 16 >= nj) return;   // whole wave past this kind's job count
    const bool act = jl < nj;
    const size_t j = jbase + jl;
    const Job jb = act ? jobs[j] : Job{0, 0, 0, 0, KIND, 0};
    int8_t *row = rows + jw * VROW;
    if (act) {   // the quad loads the block's type-5 soft bits and scrambler bytes as dwords
        const uint32_t so = src.sb_lead + (uint32_t)jb.ch * 2 * smax + jb.off;
        const __amdgpu_buffer_rsrc_t scr_r = KIND == 2 ? src.bsch_r : src.cell_r;
        const uint32_t co = KIND == 2 ? 0u : (uint32_t)jb.ch * 432;
        uint32_t *d32 = (uint32_t *)row;
        if constexpr (KIND == 0) {   // SCH/F: BKN1 = type-5 [0, 216), BKN2 = [216, 432) 268 bits on
            load_seg<54>(src.sbr, so, scr_r, co, d32, q);
            load_seg<54>(src.sbr, so + 268, scr_r, co + 4 * 54, d32 + 54, q);
        } else {
            load_seg<P.K / 4>(src.sbr, so, scr_r, co, d32, q);
        }
    }
    __syncthreads();   // the quad's row (one wave per workgroup)
    int32_t pm[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) pm[m] = (q == 0 && m == 0) ? 0 : -(1 << 28);
    const size_t gstride = 4 * ss;   // dwords between survivor groups
    uint32_t *sv = surv + 4 * j + q;
    if (act) {
        constexpr int NG = P.n2 / 8;   // n2 is a multiple of 8
        acs_groups4<NG, P.a, P.K>(pm, q, row, sv, gstride);
    }
}

// Traceback + CRC of one block per LANE (k_etsi_traceback): 64 blocks per wave, a quarter of the
// wave instructions the quad-per-block trellis waves would spend on the same serial chain (all four
// lanes of a quad followed the same path).  From state 0 (tail bits); a group's four survivor words
// ([group][job][lane]) are one 16-B load, eight groups (64 steps) in flight; the CRC over type-1 +
// CRC bits accumulates on the fly; type-1 bits go out four per dword store.
template <int KIND>
__device__ __forceinline__ void traceback_lane(const Job &jb, const uint32_t *__restrict__ sv, size_t gstride,
                                               int32_t *__restrict__ blocks, uint8_t *__restrict__ type1) {
    constexpr KindP P = kind_params(KIND);
    constexpr int NG = P.n2 / 8;
    constexpr int L = P.n1 + 16;
    static_assert(P.n1 % 4 == 0, "type-1 bits stored four per dword");
    uint32_t c = CRC_TAB.init[L];
    int s2 = 0;
    uint32_t acc = 0;
    uint8_t *ob = type1 + ((size_t)jb.ch * ETSI_MAXJ + jb.slot) * 268;
    uint32_t *op = (uint32_t *)ob;
    const bool al4 = ((uintptr_t)type1 & 3) == 0;   // a caller's device pointer may be unaligned
    for (int g0 = NG - 1; g0 >= 0; g0 -= 8) {
        uint4 w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = *(const uint4 *)(sv + (size_t)max(g0 - u, 0) * gstride);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int gi = g0 - u;
            if (gi < 0) break;
#pragma unroll
            for (int st = 7; st >= 0; --st) {
                const int t = 8 * gi + st;
                const uint32_t bit = s2 & 1;
                acc = (acc << 8) | bit;
                if ((st & 3) == 0 && t < P.n1) {   // bytes t .. t+3
                    if (al4) {
                        op[t >> 2] = acc;
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) ob[t + k] = (uint8_t)(acc >> (8 * k));
                    }
                }
                // unconditional, wave-uniform table read (scalar load, hoisted); a per-lane branch
                // around it made every step wait a global load
                const uint32_t tv = CRC_TAB.t[L - 1 - t < 0 ? 0 : L - 1 - t];
                c ^= tv & (0u - (bit & (uint32_t)(t < L)));
                // state s2's decision: word of lane s2 & 3, bit 4 st + (s2 >> 2)
                const int ln = s2 & 3;
                const uint32_t ww = ln & 2 ? (ln & 1 ? w[u].w : w[u].z) : (ln & 1 ? w[u].y : w[u].x);
                s2 = (s2 >> 1) | ((int)((ww >> (4 * st + (s2 >> 2))) & 1u) << 3);
            }
        }
    }
    int32_t *bm = blocks + ((size_t)jb.ch * ETSI_MAXJ + jb.slot) * 4;
    bm[0] = KIND;   // four dword stores: the caller's pointer need not be 16-B aligned
    bm[1] = c == 0x1D0Fu;
    bm[2] = jb.burst;
    bm[3] = jb.blk;
}

// Grid: the SCH/F region's waves, then SCH/HD's, then BSCH's (one trellis length per wave).
__global__ __launch_bounds__(64) void k_etsi_viterbi(const Job *__restrict__ jobs,
                                                     const unsigned long long *__restrict__ jcount, int C,
                                                     const int8_t *__restrict__ softbits, int smax,
                                                     const uint8_t *__restrict__ cell_scr,
                                                     const uint8_t *__restrict__ bsch_scr,
                                                     uint32_t *__restrict__ surv, int kmask) {
    __shared__ __attribute__((aligned(16))) int8_t rows[16 * VROW];
    const size_t ss = 32 * (size_t)C;
    // the soft-bit buffer [softbits, softbits + 2 C smax) from the dword holding its first byte to the
    // dword holding its last (host checks: < 4 GiB); the cell table and the BSCH table
    const uintptr_t sb0 = (uintptr_t)softbits & ~(uintptr_t)3;
    const uintptr_t sbl = ((uintptr_t)softbits + (size_t)C * 2 * smax - 1) & ~(uintptr_t)3;
    VitSrc src;
    src.sbr = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(sb0), 0, (int)(sbl - sb0 + 4), 0x00020000);
    src.cell_r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(cell_scr), 0, C * 432, 0x00020000);
    src.bsch_r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(bsch_scr), 0, 432, 0x00020000);
    src.sb_lead = (uint32_t)((uintptr_t)softbits - sb0);
    const unsigned long long cnt = *jcount;
    // kinds outside kmask are left to another launch (cell acquisition decodes BSCH first)
    const int n0 = kmask & 1 ? (int)(cnt & 0x1FFFFFull) : 0, n1 = kmask & 2 ? (int)((cnt >> 21) & 0x1FFFFFull) : 0,
              n2 = kmask & 4 ? (int)(cnt >> 42) : 0;
    // the waves the job counts need (16 blocks each), walked with a grid stride: a grid smaller
    // than that keeps the lower MAC's LDS beside the demod's bounded when the two run side by side
    const int nb0 = (n0 + 15) / 16, nb1 = (n1 + 15) / 16, nb2 = (n2 + 15) / 16;
    for (int b = blockIdx.x; b < nb0 + nb1 + nb2; b += gridDim.x) {
        if (b < nb0)
            viterbi_wave<0>(rows, jobs, n0, job_base(0, C), b, ss, src, smax, surv);
        else if (b < nb0 + nb1)
            viterbi_wave<1>(rows, jobs, n1, job_base(1, C), b - nb0, ss, src, smax, surv);
        else
            viterbi_wave<2>(rows, jobs, n2, job_base(2, C), b - nb0 - nb1, ss, src, smax, surv);
        __syncthreads();   // rows are rewritten by the next wave-batch
    }
}

// One lane per block (64 per wave), the kinds' regions one after another; grid stride as above.
__global__ __launch_bounds__(64) void k_etsi_traceback(const Job *__restrict__ jobs,
                                                       const unsigned long long *__restrict__ jcount, int C,
                                                       const uint32_t *__restrict__ surv,
                                                       int32_t *__restrict__ blocks, uint8_t *__restrict__ type1,
                                                       int kmask) {
    const size_t gstride = 4 * 32 * (size_t)C;   // dwords between survivor groups
    const unsigned long long cnt = *jcount;
    const int n[3] = {kmask & 1 ? (int)(cnt & 0x1FFFFFull) : 0, kmask & 2 ? (int)((cnt >> 21) & 0x1FFFFFull) : 0,
                      kmask & 4 ? (int)(cnt >> 42) : 0};
    const int nb0 = (n[0] + 63) / 64, nb1 = (n[1] + 63) / 64, nb2 = (n[2] + 63) / 64;
    for (int b = blockIdx.x; b < nb0 + nb1 + nb2; b += gridDim.x) {
        const int kind = b < nb0 ? 0 : b < nb0 + nb1 ? 1 : 2;
        const int jl = 64 * (b - (kind == 0 ? 0 : kind == 1 ? nb0 : nb0 + nb1)) + (int)threadIdx.x;
        if (jl >= n[kind]) continue;
        const size_t j = job_base(kind, C) + jl;
        const Job jb = jobs[j];
        const uint32_t *sv = surv + 4 * j;
        if (kind == 0) traceback_lane<0>(jb, sv, gstride, blocks, type1);
        else if (kind == 1) traceback_lane<1>(jb, sv, gstride, blocks, type1);
        else traceback_lane<2>(jb, sv, gstride, blocks, type1);
    }
}

// --------------------------------------------------------------------------- cell acquisition
// One lane per channel, after the BSCH blocks of the chunk are decoded (colour code 0): the last
// CRC-good BSCH of the channel gives its extended colour code -- MAC-SYNC colour code at type-1
// bits 4..9, D-MLE-SYNC MCC at 31..40 and MNC at 41..54 (EN 300 392-2 §21.4.4.2, §18.4.2.1) -- and
// the scrambling init (ecc << 2) | 3 (§8.2.5.2).  Without one the channel keeps its init.  The
// channel's 432 scrambler bytes (the table k_etsi_viterbi descrambles with) are regenerated only
// when the init differs from the one the table was made for (tab_init; 0 = none yet).

__global__ __launch_bounds__(256) void k_cell_acquire(int C, const int32_t *__restrict__ nburst,
                                                      const int32_t *__restrict__ bursts,
                                                      const int32_t *__restrict__ blocks,
                                                      const uint8_t *__restrict__ type1, uint32_t *__restrict__ cell_init,
                                                      uint32_t *__restrict__ tab_init, uint8_t *__restrict__ cell_scr) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= C) return;
    uint32_t init = cell_init[ch];
    const int nb = min(nburst[ch], ETSI_MAXB);
    int q = 0;   // block slot of burst b: the sync kernel's numbering (1 per NDB(n), 2 per NDB(p) / SB)
    for (int b = 0; b < nb; ++b) {
        const int k = bursts[((size_t)ch * ETSI_MAXB + b) * 2 + 1];
        if (k == 2 && q < ETSI_MAXJ && blocks[((size_t)ch * ETSI_MAXJ + q) * 4 + 1]) {
            const uint8_t *t = type1 + ((size_t)ch * ETSI_MAXJ + q) * 268;
            uint32_t ecc = 0;
            for (int i = 4; i < 10; ++i) ecc = (ecc << 1) | (t[i] & 1u);     // colour code (low 6)
            uint32_t mm = 0;
            for (int i = 31; i < 55; ++i) mm = (mm << 1) | (t[i] & 1u);     // MCC(10) MNC(14)
            init = (((mm << 6) | ecc) << 2) | 3u;
        }
        q += k == 0 ? 1 : 2;
    }
    cell_init[ch] = init;
    if (tab_init[ch] != init) {
        tab_init[ch] = init;
        uint32_t r = init;
        uint32_t *o = reinterpret_cast<uint32_t *>(cell_scr + (size_t)ch * 432);
        for (int w = 0; w < 108; ++w) {   // four scrambler bytes (0 / 1) per dword store
            uint32_t v = 0;
            for (int k = 0; k < 4; ++k) {
                const uint32_t bt = (uint32_t)__popc(r & SCR_TAPS) & 1u;
                r = (r >> 1) | (bt << 31);
                v |= bt << (8 * k);
            }
            o[w] = v;
        }
    }
}

// --------------------------------------------------------------------------- grouped cell acquisition
// The scrambler is linear over GF(2): with x[0..31] the init's bits and x[n + 32] = XOR over the
// taps t of x[n + t], its output bit n is x[n + 32] = parity(init & SCR_MASK.w[n]).  The table lets
// a wave form all 432 bits at once (a lane four of them) where k_cell_acquire steps the register.

// One WAVE per group of G rows (tetra_lmac_etsi_acquire_groups), after the BSCH blocks of every row
// are decoded: k_cell_acquire's rule over the group's rows in ascending order and each row's bursts
// in order.  Lane i of a step looks at (row i >> 3, burst i & 7); a ballot counts the CRC-good BSCH
// blocks and names the last one, whose type-1 fields a second ballot packs into the init (lane j
// reads the bit that lands at bit j).  The group's scrambler sequence is formed once (SCR_MASK, a
// lane's dwords w = lane and lane + 64) and stored as whole dwords to the 432-byte table row of every
// row of the group whose tab_init differs: the table stays per row, as k_etsi_viterbi reads it.
constexpr int ACQ_WAVES = 4;   // groups per workgroup (the waves share nothing)

__global__ __launch_bounds__(64 * ACQ_WAVES) void k_cell_acquire_groups(
    int NG, int G, const int32_t *__restrict__ nburst, const int32_t *__restrict__ bursts,
    const int32_t *__restrict__ blocks, const uint8_t *__restrict__ type1, uint32_t *__restrict__ cell_init /*[NG]*/,
    int32_t *__restrict__ ngood /*[NG]*/, uint32_t *__restrict__ tab_init /*[NG G]*/, uint8_t *__restrict__ cell_scr) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * ACQ_WAVES + (threadIdx.x >> 6);
    if (g >= NG) return;   // the whole wave
    const size_t row0 = (size_t)g * G;
    // block slot of burst b of a row: the sync kernel's numbering (1 per NDB(n), 2 per NDB(p) / SB)
    auto slot_of = [&](size_t ch, int b) {
        int q = 0;
        for (int p = 0; p < b; ++p) q += bursts[(ch * ETSI_MAXB + p) * 2 + 1] == 0 ? 1 : 2;
        return q;
    };
    int good = 0, last = -1;   // wave-uniform: CRC-good BSCH blocks, the last one's (row, burst) index
    for (int i0 = 0; i0 < ETSI_MAXB * G; i0 += 64) {
        const int i = i0 + lane, r = i / ETSI_MAXB, b = i % ETSI_MAXB;
        bool ok = false;
        if (r < G) {
            const size_t ch = row0 + r;
            if (b < min(nburst[ch], ETSI_MAXB) && bursts[(ch * ETSI_MAXB + b) * 2 + 1] == 2) {
                const int q = slot_of(ch, b);
                ok = q < ETSI_MAXJ && blocks[(ch * ETSI_MAXJ + q) * 4 + 1] != 0;
            }
        }
        const unsigned long long bal = __ballot(ok);
        if (bal) {
            good += __popcll(bal);
            last = i0 + 63 - __clzll((long long)bal);
        }
    }
    uint32_t init = cell_init[g];
    if (last >= 0) {
        const size_t ch = row0 + last / ETSI_MAXB;
        const uint8_t *t = type1 + (ch * ETSI_MAXJ + slot_of(ch, last % ETSI_MAXB)) * 268;
        // lanes 0..5: colour code bit j = type-1 bit 9 - j; lanes 8..31: bit j - 8 of MCC(10) MNC(14),
        // type-1 bit 62 - j (the fields are MSB first)
        const bool use = lane < 6 || (lane >= 8 && lane < 32);
        const uint32_t bit = use ? t[lane < 6 ? 9 - lane : 62 - lane] & 1u : 0u;
        const unsigned long long f = __ballot(bit != 0);
        const uint32_t ecc = (uint32_t)f & 0x3Fu, mm = (uint32_t)(f >> 8) & 0xFFFFFFu;
        init = (((mm << 6) | ecc) << 2) | 3u;
    }
    if (lane == 0) {
        cell_init[g] = init;
        ngood[g] = good;
    }
    uint32_t v0 = 0, v1 = 0;   // the sequence's dwords lane and 64 + lane (four 0 / 1 bytes each)
    bool have = false;
    for (int r0 = 0; r0 < G; r0 += 64) {
        const int r = r0 + lane;
        const bool need = r < G && tab_init[row0 + r] != init;
        unsigned long long m = __ballot(need);
        if (m && !have) {
            auto dword = [&](int w) {
                const uint4 k = *reinterpret_cast<const uint4 *>(&SCR_MASK.w[4 * w]);
                return ((uint32_t)__popc(init & k.x) & 1u) | (((uint32_t)__popc(init & k.y) & 1u) << 8) |
                       (((uint32_t)__popc(init & k.z) & 1u) << 16) | (((uint32_t)__popc(init & k.w) & 1u) << 24);
            };
            v0 = dword(lane);
            v1 = dword(min(lane + 64, 107));
            have = true;
        }
        if (need) tab_init[row0 + r] = init;
        while (m) {   // wave-uniform: one coalesced 432-byte store per row
            const int rr = r0 + __ffsll((long long)m) - 1;
            m &= m - 1;
            uint32_t *o = reinterpret_cast<uint32_t *>(cell_scr + (row0 + rr) * 432);
            o[lane] = v0;
            if (lane < 44) o[64 + lane] = v1;
        }
    }
}

// --------------------------------------------------------------------------- component kernels
// Block decode of F independent blocks of one kind (16 lanes per block, 4 per wave).
__global__ __launch_bounds__(64) void k_decode_blocks(const int8_t *__restrict__ soft5, int F, int kind,
                                                      const uint8_t *__restrict__ scr /*[F][K]*/,
                                                      uint8_t *__restrict__ type1, uint8_t *__restrict__ crc_ok) {
    __shared__ __attribute__((aligned(16))) int8_t ms[4][4 * 288];
    __shared__ uint64_t surv[288];
    __shared__ uint8_t t2[4][288];
    const int lane = threadIdx.x, g = lane >> 4, st = lane & 15;
    const int j = blockIdx.x * 4 + g;
    const bool act = j < F;
    const KindP P = kind_params(kind);
    for (int i = st; i < 4 * P.n2; i += 16) ms[g][i] = 0;
    __syncthreads();
    if (act) {
        for (int i = 1 + st; i <= P.K; i += 16) {
            const int k = 1 + (int)(((long)P.a * i) % P.K);
            const int8_t v = soft5[(size_t)j * P.K + k - 1];
            ms[g][punct_index(i) - 1] = scr[(size_t)j * P.K + k - 1] ? (int8_t)(-v) : v;
        }
    }
    __syncthreads();
    int32_t pm = st == 0 ? 0 : -(1 << 28);
    const int b = st & 1, d0 = (st >> 1) & 1, d1 = (st >> 2) & 1, d2 = (st >> 3) & 1;
    for (int t = 0; t < P.n2; ++t) {
        const int8_t *m = ms[g] + 4 * t;
        const int32_t m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3];
        const int32_t v0 = ((b ^ d0) ? -m0 : m0) + ((b ^ d1 ^ d2) ? -m1 : m1) + ((b ^ d0 ^ d1) ? -m2 : m2) +
                           ((b ^ d0 ^ d2) ? -m3 : m3);
        const int32_t a0 = __shfl(pm, (lane & ~15) + (st >> 1), 64) + v0;
        const int32_t a1 = __shfl(pm, (lane & ~15) + ((st >> 1) | 8), 64) - v0;
        const bool take1 = a1 > a0;
        const unsigned long long sv = __ballot(take1);
        pm = take1 ? a1 : a0;
        if (lane == 0) surv[t] = sv;
    }
    __syncthreads();
    if (act && st == 0) {
        int s2 = 0;
        for (int t = P.n2 - 1; t >= 0; --t) {
            t2[g][t] = (uint8_t)(s2 & 1);
            s2 = (s2 >> 1) | ((int)((surv[t] >> (16 * g + s2)) & 1ull) << 3);
        }
        uint32_t c = 0xFFFF;
        for (int i = 0; i < P.n1 + 16; ++i) {
            c ^= (uint32_t)t2[g][i] << 15;
            c = (c & 0x8000u) ? ((c << 1) ^ 0x1021u) : (c << 1);
            c &= 0xFFFFu;
        }
        crc_ok[j] = c == 0x1D0Fu;
    }
    __syncthreads();
    if (act)
        for (int i = st; i < P.n1; i += 16) type1[(size_t)j * P.n1 + i] = t2[g][i];
}

// Encoder type-1 -> type-5 (one block per thread; CRC, tail, mother code, puncture, interleave, scramble)
__global__ void k_encode_blocks(const uint8_t *__restrict__ type1, int F, int kind, const uint8_t *__restrict__ scr,
                                uint8_t *__restrict__ type5) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= F) return;
    const KindP P = kind_params(kind);
    const uint8_t *in = type1 + (size_t)j * P.n1;
    uint8_t t2[288];
    uint32_t c = 0xFFFF;
    for (int i = 0; i < P.n1; ++i) {
        t2[i] = in[i] & 1;
        c ^= (uint32_t)t2[i] << 15;
        c = (c & 0x8000u) ? ((c << 1) ^ 0x1021u) : (c << 1);
        c &= 0xFFFFu;
    }
    c ^= 0xFFFFu;
    for (int k = 0; k < 16; ++k) t2[P.n1 + k] = (c >> (15 - k)) & 1u;
    for (int k = 0; k < 4; ++k) t2[P.n1 + 16 + k] = 0;
    for (int i = 1; i <= P.K; ++i) {
        const int mi = punct_index(i) - 1;   // mother index: step mi/4, generator mi%4
        const int step = mi >> 2, gen = mi & 3;
        const uint32_t bb = t2[step];
        const uint32_t e0 = step >= 1 ? t2[step - 1] : 0, e1 = step >= 2 ? t2[step - 2] : 0,
                       e2 = step >= 3 ? t2[step - 3] : 0, e3 = step >= 4 ? t2[step - 4] : 0;
        uint32_t v = gen == 0 ? (bb ^ e0 ^ e3) : gen == 1 ? (bb ^ e1 ^ e2 ^ e3) : gen == 2 ? (bb ^ e0 ^ e1 ^ e3)
                                                                                          : (bb ^ e0 ^ e2 ^ e3);
        const int k = 1 + (int)(((long)P.a * i) % P.K);
        type5[(size_t)j * P.K + k - 1] = (uint8_t)(v ^ scr[(size_t)j * P.K + k - 1]);
    }
}

}  // namespace

// --------------------------------------------------------------------------- host side
static void scramble_seq(uint32_t r, int n, uint8_t *out) {
    for (int i = 0; i < n; ++i) {
        const uint32_t b = ((r >> 0) ^ (r >> 6) ^ (r >> 9) ^ (r >> 10) ^ (r >> 16) ^ (r >> 20) ^ (r >> 21) ^ (r >> 22) ^
                            (r >> 24) ^ (r >> 25) ^ (r >> 27) ^ (r >> 28) ^ (r >> 30) ^ (r >> 31)) & 1u;
        r = (r >> 1) | (b << 31);
        out[i] = (uint8_t)b;
    }
}

// n scrambler inits (host or device memory) -> tab: their sequences, K bytes (0 / 1) each.
static int scramble_table(tetra_ctx *ctx, const uint32_t *inits, size_t n, int K, std::vector<uint8_t> &tab) {
    std::vector<uint32_t> init(n);
    HIP_TRY(ctx, hipMemcpy(init.data(), inits, n * 4, hipMemcpyDefault));
    tab.resize(n * K);
    for (size_t i = 0; i < n; ++i) scramble_seq(init[i], K, tab.data() + i * K);
    return TETRA_OK;
}

// The cell table of C channels: C scrambler rows of 432 bytes and the BSCH row (colour code 0) in
// S_W5, and in S_W14 the inits the rows hold (cell acquisition regenerates a row whose init changed).
// inits == nullptr: an empty table (inits 0 = none yet), only the BSCH row written.
static int ensure_cells(tetra_ctx *ctx, const uint32_t *inits, size_t C) {
    std::vector<uint8_t> tab;
    if (inits) {
        const int rc = scramble_table(ctx, inits, C, 432, tab);
        if (rc) return rc;
    }
    const size_t rows = tab.size();   // C * 432, or 0
    tab.resize(rows + 432);
    scramble_seq(3u, 432, tab.data() + rows);
    uint8_t *d = (uint8_t *)ws(ctx, S_W5, C * 432 + 432);
    uint32_t *ti = (uint32_t *)ws(ctx, S_W14, C * 4);
    if (!d || !ti) return TETRA_E_NOMEM;
    HIP_TRY(ctx, hipMemcpyAsync(d + C * 432 - rows, tab.data(), tab.size(), hipMemcpyHostToDevice, ctx->stream));
    if (inits)
        HIP_TRY(ctx, hipMemcpyAsync(ti, inits, C * 4, hipMemcpyDefault, ctx->stream));
    else
        HIP_TRY(ctx, hipMemsetAsync(ti, 0, C * 4, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // tab is a pageable host buffer
    ctx->cells = C;
    return TETRA_OK;
}

extern "C" {

int tetra_etsi_set_cells(tetra_ctx *ctx, const uint32_t *scramb_init, size_t C) {
    if (!ctx || !scramb_init || C == 0) return TETRA_E_INVALID;
    return ensure_cells(ctx, scramb_init, C);
}

int tetra_etsi_decode_blocks(tetra_ctx *ctx, const int8_t *soft5, size_t F, int kind, const uint32_t *scramb_init,
                             uint8_t *type1, uint8_t *crc_ok) {
    if (!ctx || kind < 0 || kind > 2) return TETRA_E_INVALID;
    if (F == 0) return TETRA_OK;
    const KindP P = kind_params(kind);
    std::vector<uint8_t> tab;
    if (int rc = scramble_table(ctx, scramb_init, F, P.K, tab)) return rc;
    Staging st(ctx);
    const int8_t *s = (const int8_t *)st.in(soft5, F * P.K);
    const uint8_t *scr = (const uint8_t *)st.in(tab.data(), tab.size());
    uint8_t *t = (uint8_t *)st.out(type1, F * P.n1);
    uint8_t *o = (uint8_t *)st.out(crc_ok, F);
    if (!s || !scr || !t || !o) return st.finish();
    {
        PROF(ctx, "etsi_decode_blocks");
        hipLaunchKernelGGL(k_decode_blocks, dim3((unsigned)((F + 3) / 4)), dim3(64), 0, ctx->stream, s, (int)F, kind,
                           scr, t, o);
    }
    return st.finish();
}

int tetra_etsi_encode_blocks(tetra_ctx *ctx, const uint8_t *type1, size_t F, int kind, const uint32_t *scramb_init,
                             uint8_t *type5) {
    if (!ctx || kind < 0 || kind > 2) return TETRA_E_INVALID;
    if (F == 0) return TETRA_OK;
    const KindP P = kind_params(kind);
    std::vector<uint8_t> tab;
    if (int rc = scramble_table(ctx, scramb_init, F, P.K, tab)) return rc;
    Staging st(ctx);
    const uint8_t *t = (const uint8_t *)st.in(type1, F * P.n1);
    const uint8_t *scr = (const uint8_t *)st.in(tab.data(), tab.size());
    uint8_t *o = (uint8_t *)st.out(type5, F * P.K);
    if (!t || !scr || !o) return st.finish();
    hipLaunchKernelGGL(k_encode_blocks, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, ctx->stream, t, (int)F, kind, scr,
                       o);
    return st.finish();
}

// The lower MAC's launch sequence; cell_init (device) selects acquisition, else the configured cells.
// G > 0 (with ngood): acquisition per group of G rows, cell_init and ngood C / G long.
// score (with cap; agree may be null): the vote (etsi_vote.hip) in place of the last-good-BSCH kernels,
// over groups of G rows, or of one row where G == 0; score and agree as long as cell_init.
static int lmac_etsi(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, const int32_t *nsym, size_t C,
                     size_t smax, uint32_t *cell_init, int32_t *nburst, int32_t *bursts, int32_t *nblock,
                     int32_t *blocks, uint8_t *type1, int32_t *lead = nullptr, int8_t *next_soft = nullptr,
                     uint8_t *next_hard = nullptr, size_t G = 0, int32_t *ngood = nullptr, int32_t *score = nullptr,
                     int32_t cap = 0, int32_t *agree = nullptr) {
    if (!ctx || C == 0) return TETRA_E_INVALID;
    const size_t ncell = G ? C / G : C;   // acquisition states
    if (!cell_init && ctx->cells < C)
        return tetra_fail(ctx, TETRA_E_INVALID, "tetra_etsi_set_cells() for %zu channels first", C);
    if (2 * smax > LMAC_MAXBITS + 4) return tetra_fail(ctx, TETRA_E_INVALID, "chunk too long for tetra_lmac_etsi");
    // k_etsi_viterbi reads the soft bits and the cell table through 32-bit buffer offsets
    if (C * smax * 2 + 8 > (size_t)INT32_MAX || (C + 1) * 432 > (size_t)INT32_MAX)
        return tetra_fail(ctx, TETRA_E_INVALID, "too many channels for one tetra_lmac_etsi call (%zu)", C);
    Staging st(ctx);
    uint32_t *ci = cell_init ? (uint32_t *)st.inout(cell_init, ncell * 4) : nullptr;
    int32_t *ngo = G ? (int32_t *)st.out(ngood, ncell * 4) : nullptr;
    // the vote's score (in/out) and agree (out): host arrays travel as one staged buffer (the streaming
    // form stages nine outputs already)
    int32_t *sco = score, *ago = agree;
    std::vector<int32_t> small;
    const bool hs = score && !is_device_ptr(score), ha = agree && !is_device_ptr(agree);
    if (hs || ha) {
        small.assign((hs ? ncell : 0) + (ha ? ncell : 0), 0);
        if (hs) memcpy(small.data(), score, ncell * 4);
        int32_t *d = (int32_t *)st.inout(small.data(), small.size() * 4);
        if (!d) return st.finish();
        if (hs) sco = d;
        if (ha) ago = d + (hs ? ncell : 0);
    }
    // streaming into the input rows themselves: host rows are staged in and back out (with the tail)
    const bool alias = lead && next_soft == softbits;
    const int8_t *sb = alias ? (const int8_t *)st.inout(const_cast<int8_t *>(softbits), C * smax * 2)
                             : (const int8_t *)st.in(softbits, C * smax * 2);
    const uint8_t *hd = alias ? (const uint8_t *)st.inout(const_cast<uint8_t *>(hard), C * smax)
                              : (const uint8_t *)st.in(hard, C * smax);
    // streaming: the scan state and the rows the tail goes to
    int32_t *ld_ = lead ? (int32_t *)st.inout(lead, C * 4) : nullptr;
    int8_t *nsb = nullptr;
    uint8_t *nhd = nullptr;
    if (lead) {
        nsb = next_soft == softbits ? const_cast<int8_t *>(sb) : (int8_t *)st.inout(next_soft, C * smax * 2);
        nhd = next_hard == hard ? const_cast<uint8_t *>(hd) : (uint8_t *)st.inout(next_hard, C * smax);
        if (!ld_ || !nsb || !nhd) return st.finish();
    }
    const int32_t *ns = (const int32_t *)st.in(nsym, C * 4);
    int32_t *nbo = (int32_t *)st.out(nburst, C * 4);
    int32_t *bo = (int32_t *)st.out(bursts, C * ETSI_MAXB * 2 * 4);
    int32_t *nko = (int32_t *)st.out(nblock, C * 4);
    int32_t *ko = (int32_t *)st.out(blocks, C * ETSI_MAXJ * 4 * 4);
    uint8_t *to = (uint8_t *)st.out(type1, C * ETSI_MAXJ * 268);
    const size_t jtot = 32 * C;   // the three job regions (job_base / job_cap)
    // workspace: [job counters per kind (16 B)] [jobs] [survivors: 36 groups x jtot x 4 lanes x 32 bits
    // (SCH/F: 288 steps / 8; allocated as 288 x jtot dwords)]
    char *w = (char *)ws(ctx, S_W7, 16 + jtot * sizeof(Job) + 288 * jtot * 4 + (lead ? 8 * C : 0));
    if ((cell_init && !ci) || (G && !ngo) || !sb || !hd || !ns || !nbo || !bo || !nko || !ko || !to || !w) return st.finish();
    unsigned long long *jcount = (unsigned long long *)w;
    Job *jobs = (Job *)(w + 16);
    uint32_t *surv = (uint32_t *)(w + 16 + jtot * sizeof(Job));
    int32_t *tinfo = lead ? (int32_t *)(w + 16 + jtot * sizeof(Job) + 288 * jtot * 4) : nullptr;   // streaming
    if (cell_init && ctx->cells != C) {   // acquisition on a new channel count: an empty table
        const int rc = ensure_cells(ctx, nullptr, C);
        if (rc) return rc;
    }
    uint8_t *cells = (uint8_t *)ctx->slot[S_W5].p;
    const uint8_t *bsch_scr = cells + ctx->cells * 432;
    {
        PROF(ctx, "etsi_sync");
        HIP_TRY(ctx, hipMemsetAsync(jcount, 0, 16, ctx->stream));
        const unsigned ngrp = (unsigned)((C + SYNC_WAVES - 1) / SYNC_WAVES);
        // double-buffered rows: the sync kernel moves the tails itself (no k_etsi_tail launch)
        const bool other = lead && nhd != hd;
        hipLaunchKernelGGL(k_etsi_sync, dim3(ngrp), dim3(64 * SYNC_WAVES), 0,
                           ctx->stream, hd, ns, (int)smax, nbo, bo, nko, jcount, jobs, (int)C, ld_,
                           lead ? TETRA_ETSI_RESERVE : 0, tinfo, sb, other ? nhd : nullptr, other ? nsb : nullptr);
    }
    // grids: the waves each kind's job capacity needs (16 blocks per trellis wave, 64 per traceback wave)
    // (TETRA_LMAC_GRID_CAP: at most that many trellis workgroups, a quarter as many traceback ones --
    // the kernels walk their jobs with a grid stride; 0 = the capacity)
    static const long gcap = getenv("TETRA_LMAC_GRID_CAP") ? atol(getenv("TETRA_LMAC_GRID_CAP")) : 0;
    auto vgrid = [&](int m) {
        size_t g = 0;
        for (int k = 0; k < 3; ++k) g += (m >> k) & 1 ? (job_cap(k, C) + 15) / 16 : 0;
        if (gcap > 0 && g > (size_t)gcap) g = (size_t)gcap;
        return dim3((unsigned)g);
    };
    auto tgrid = [&](int m) {
        size_t g = 0;
        for (int k = 0; k < 3; ++k) g += (m >> k) & 1 ? (job_cap(k, C) + 63) / 64 : 0;
        if (gcap > 0 && g > (size_t)(gcap / 4 + 1)) g = (size_t)(gcap / 4 + 1);
        return dim3((unsigned)g);
    };
    int mask = 7;
    if (ci) {   // BSCH first (colour code 0), then the cell from it, then SCH/F + SCH/HD
        PROF(ctx, "etsi_acquire");
        hipLaunchKernelGGL(k_etsi_viterbi, vgrid(4), dim3(64), 0, ctx->stream, jobs, jcount, (int)C, sb, (int)smax,
                           cells, bsch_scr, surv, 4);
        hipLaunchKernelGGL(k_etsi_traceback, tgrid(4), dim3(64), 0, ctx->stream, jobs, jcount, (int)C, surv, ko, to, 4);
        if (sco)
            launch_cell_vote(ctx, ncell, G ? G : 1, sb, 2 * smax, lead ? 2 * TETRA_ETSI_RESERVE : 0, nbo, bo, ko, to, ci,
                             sco, cap, ngo, ago, (uint32_t *)ctx->slot[S_W14].p, cells);
        else if (G)
            hipLaunchKernelGGL(k_cell_acquire_groups, dim3(grid_for(ncell, ACQ_WAVES)), dim3(64 * ACQ_WAVES), 0,
                               ctx->stream, (int)ncell, (int)G, nbo, bo, ko, to, ci, ngo,
                               (uint32_t *)ctx->slot[S_W14].p, cells);
        else
            hipLaunchKernelGGL(k_cell_acquire, dim3(grid_for(C, 256)), dim3(256), 0, ctx->stream, (int)C, nbo, bo, ko,
                               to, ci, (uint32_t *)ctx->slot[S_W14].p, cells);
        mask = 3;
    }
    {
        PROF(ctx, "etsi_viterbi");
        hipLaunchKernelGGL(k_etsi_viterbi, vgrid(mask), dim3(64), 0, ctx->stream, jobs, jcount, (int)C, sb, (int)smax,
                           cells, bsch_scr, surv, mask);
    }
    {
        PROF(ctx, "etsi_traceback");
        hipLaunchKernelGGL(k_etsi_traceback, tgrid(mask), dim3(64), 0, ctx->stream, jobs, jcount, (int)C, surv, ko, to,
                           mask);
    }
    if (lead && nhd == hd) {   // these rows: the tails after the trellis has read them
        PROF(ctx, "etsi_tail");
        hipLaunchKernelGGL(k_etsi_tail, dim3((unsigned)C), dim3(64), 0, ctx->stream, hd, sb, (int)smax, (int)C, tinfo,
                           TETRA_ETSI_RESERVE, nhd, nsb, ld_);
    }
    const int rc = st.finish();
    if (rc == TETRA_OK && hs) memcpy(score, small.data(), ncell * 4);
    if (rc == TETRA_OK && ha) memcpy(agree, small.data() + (hs ? ncell : 0), ncell * 4);
    return rc;
}

int tetra_lmac_etsi(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, const int32_t *nsym, size_t C,
                    size_t smax, int32_t *nburst, int32_t *bursts, int32_t *nblock, int32_t *blocks, uint8_t *type1) {
    return lmac_etsi(ctx, softbits, hard, nsym, C, smax, nullptr, nburst, bursts, nblock, blocks, type1);
}

int tetra_lmac_etsi_acquire(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, const int32_t *nsym,
                            size_t C, size_t smax, uint32_t *cell_init, int32_t *nburst, int32_t *bursts,
                            int32_t *nblock, int32_t *blocks, uint8_t *type1) {
    if (!cell_init) return tetra_fail(ctx, TETRA_E_INVALID, "cell_init is NULL");
    return lmac_etsi(ctx, softbits, hard, nsym, C, smax, cell_init, nburst, bursts, nblock, blocks, type1);
}

int tetra_lmac_etsi_acquire_groups(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, const int32_t *nsym,
                                   size_t C, size_t smax, size_t G, uint32_t *cell_init, int32_t *ngood,
                                   int32_t *nburst, int32_t *bursts, int32_t *nblock, int32_t *blocks,
                                   uint8_t *type1) {
    if (!cell_init || !ngood) return tetra_fail(ctx, TETRA_E_INVALID, "cell_init or ngood is NULL");
    if (G == 0 || C % G != 0)
        return tetra_fail(ctx, TETRA_E_INVALID, "lmac_etsi_acquire_groups: %zu rows are not whole groups of %zu", C, G);
    return lmac_etsi(ctx, softbits, hard, nsym, C, smax, cell_init, nburst, bursts, nblock, blocks, type1, nullptr,
                     nullptr, nullptr, G, ngood);
}

int tetra_lmac_etsi_vote_groups(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, const int32_t *nsym,
                                size_t C, size_t smax, size_t G, int32_t cap, uint32_t *cell_init, int32_t *score,
                                int32_t *ngood, int32_t *agree, int32_t *nburst, int32_t *bursts, int32_t *nblock,
                                int32_t *blocks, uint8_t *type1) {
    if (!cell_init || !score || !ngood || !agree)
        return tetra_fail(ctx, TETRA_E_INVALID, "lmac_etsi_vote_groups: cell_init, score, ngood or agree is NULL");
    if (cap <= 0) return tetra_fail(ctx, TETRA_E_INVALID, "lmac_etsi_vote_groups: cap %d is not positive", (int)cap);
    if (G == 0 || C % G != 0 || G > VOTE_MAXG)
        return tetra_fail(ctx, TETRA_E_INVALID, "lmac_etsi_vote_groups: %zu rows are not whole groups of %zu (at most %zu)",
                          C, G, VOTE_MAXG);
    return lmac_etsi(ctx, softbits, hard, nsym, C, smax, cell_init, nburst, bursts, nblock, blocks, type1, nullptr,
                     nullptr, nullptr, G, ngood, score, cap, agree);
}

int tetra_lmac_etsi_stream(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, const int32_t *nsym,
                           size_t C, size_t stride, int32_t *lead, int8_t *next_soft, uint8_t *next_hard,
                           uint32_t *cell_init, int32_t *nburst, int32_t *bursts, int32_t *nblock, int32_t *blocks,
                           uint8_t *type1) {
    if (!lead || !next_soft || !next_hard || stride <= TETRA_ETSI_RESERVE)
        return tetra_fail(ctx, TETRA_E_INVALID, "lmac_etsi_stream: lead, next rows and stride > TETRA_ETSI_RESERVE");
    if ((next_soft == softbits) != (next_hard == hard))
        return tetra_fail(ctx, TETRA_E_INVALID, "lmac_etsi_stream: next rows must both alias the inputs or neither");
    return lmac_etsi(ctx, softbits, hard, nsym, C, stride, cell_init, nburst, bursts, nblock, blocks, type1, lead,
                     next_soft, next_hard);
}

int tetra_lmac_etsi_stream_vote(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, const int32_t *nsym,
                                size_t C, size_t stride, int32_t *lead, int8_t *next_soft, uint8_t *next_hard,
                                int32_t cap, uint32_t *cell_init, int32_t *score, int32_t *agree, int32_t *nburst,
                                int32_t *bursts, int32_t *nblock, int32_t *blocks, uint8_t *type1) {
    if (!lead || !next_soft || !next_hard || stride <= TETRA_ETSI_RESERVE)
        return tetra_fail(ctx, TETRA_E_INVALID, "lmac_etsi_stream_vote: lead, next rows and stride > TETRA_ETSI_RESERVE");
    if ((next_soft == softbits) != (next_hard == hard))
        return tetra_fail(ctx, TETRA_E_INVALID, "lmac_etsi_stream_vote: next rows must both alias the inputs or neither");
    if (!cell_init || !score) return tetra_fail(ctx, TETRA_E_INVALID, "lmac_etsi_stream_vote: cell_init or score is NULL");
    if (cap <= 0) return tetra_fail(ctx, TETRA_E_INVALID, "lmac_etsi_stream_vote: cap %d is not positive", (int)cap);
    return lmac_etsi(ctx, softbits, hard, nsym, C, stride, cell_init, nburst, bursts, nblock, blocks, type1, lead,
                     next_soft, next_hard, 0, nullptr, score, cap, agree);
}

}  // extern "C"
