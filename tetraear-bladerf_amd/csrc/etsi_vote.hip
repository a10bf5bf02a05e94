// etsi_vote.hip -- the lower MAC's cell vote on gfx950 (tetra_lmac_etsi_vote_groups, _stream_vote): where
// k_cell_acquire_groups lets the last CRC-good BSCH of a group set its scrambling init, every CRC-good
// BSCH votes with the correlation of its soft bits with the codeword the decoder chose, and the
// incumbent cell defends with the score it has gathered.  The rule is in include/tetra_hip.h and,
// restated with the oracle, in tests/_lmac_vote.py.
//
//   k_cell_vote_groups  one wave per group of G <= 32 rows.  The ballot walk of k_cell_acquire_groups
//               finds the CRC-good BSCH blocks; for each, in order, the whole wave works on the one
//               block: a ballot packs its 60 type-1 bits into a word, the CRC-16 comes from the linear
//               table as an XOR reduction, lanes form type-5 bits `lane` and `lane + 64` (inverse
//               interleaver, puncturer, mother code as a parity over a 5-bit window, scrambler bit of
//               init 3) and hold them against the soft bytes the trellis read; (init, weight) go to the
//               wave's LDS list.  The tally takes each distinct init's total by compare + reduction
//               over the list, lane k owning ballots k, k + 64, ...  The tail -- the winner's scrambler
//               sequence stored to the rows whose tab_init differs -- restates k_cell_acquire_groups's.
#include "etsi_vote.h"
#include "etsi_coding.h"

namespace {

constexpr int VOTE_WAVES = 4;                              // groups per workgroup (the waves share nothing)
constexpr int VOTE_MAXBAL = (int)VOTE_MAXG * ETSI_MAXB;    // ballots of a group: every burst a CRC-good BSCH
static_assert(TETRA_ETSI_MAXB == ETSI_MAXB && TETRA_ETSI_MAXJ == ETSI_MAXJ, "record layout");
static_assert(VOTE_MAXBAL * 128 * 120 < (1 << 23) && VOTE_MAXBAL < (1 << 9), "a total and a count share a dword");

// 11^-1 mod 120: type-5 position p = 11 i mod 120 holds type-3 bit i = AINV p mod 120 (0 -> 120)
constexpr int inv_mod(int a, int K) {
    for (int x = 1; x < K; ++x)
        if ((long)a * x % K == 1) return x;
    return 0;
}
constexpr KindP BSCH = kind_params(2);
constexpr int AINV = inv_mod(BSCH.a, BSCH.K);
static_assert(AINV != 0 && BSCH.n1 == 60 && BSCH.n2 == 80 && BSCH.K == 120, "BSCH: 60 -> 80 -> 120 bits");

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v ^= (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

// What a lane needs of the tables for every block, read once per wave: the CRC table word of type-1 bit
// `lane`, and for its type-5 positions p = lane and lane + 64 the trellis step of the bit, its
// generator's taps and the scrambler bit of init 3.
struct LaneTab {
    uint32_t crc_t;
    int step[2];
    uint32_t taps[2], scr[2];
};
__device__ __forceinline__ LaneTab lane_tab(int lane) {
    LaneTab k;
    k.crc_t = CRC_TAB.t[max(BSCH.n1 - 1 - lane, 0)];   // type-1 bit j sits 59 - j from the end
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int p = min(lane + 64 * u, BSCH.K - 1);
        // type-3 bit i = 3 t3 + r + 1 is mother bit 8 t3 + (0, 1, 4)[r] (punct_index): trellis step
        // 2 t3 + (r == 2), generator G2 for r == 1, else G1 (taps on the window: bit 4 = the step's bit)
        const int i3 = AINV * p % BSCH.K;
        const int ti = (i3 == 0 ? BSCH.K : i3) - 1, t3 = ti / 3, r = ti - 3 * t3;
        k.step[u] = 2 * t3 + (r == 2);
        k.taps[u] = r == 1 ? 0x17u : 0x19u;
        k.scr[u] = (uint32_t)__popc(3u & SCR_MASK.w[p]) & 1u;
    }
    return k;
}

// The weight of one CRC-good BSCH block (the whole wave; t, srow, p0 wave-uniform): its type-1 bytes t
// re-encoded with init 3 against the 120 soft bytes from srow[p0] (row bits outside [0, row_bits) read
// as 0): max(1, WSUM - 2 WERR) of tetra_etsi_link_quality's block record.  The loads -- a type-1 byte and
// two soft bytes per lane -- depend on nothing computed here, so they are in flight together.
__device__ __forceinline__ int32_t bsch_weight(const uint8_t *__restrict__ t, const int8_t *__restrict__ srow, long p0,
                                               long row_bits, int lane, const LaneTab &k) {
    int s[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const long pos = p0 + lane + 64 * u;
        s[u] = lane + 64 * u < BSCH.K && pos >= 0 && pos < row_bits ? srow[pos] : 0;
    }
    // type-2 bits: 60 type-1 bits by a ballot, 16 CRC bits, 4 zero tail bits
    const uint32_t bit = lane < BSCH.n1 ? t[lane] & 1u : 0u;
    const uint64_t t1 = __ballot(bit != 0);
    const uint32_t x = bit ? k.crc_t : 0u;
    const uint32_t crc = (wave_xor(x) ^ CRC_TAB.init[BSCH.n1] ^ 0xFFFFu) & 0xFFFFu;
    const uint64_t rev = __brev(crc) >> 16;   // bit k = CRC bit 15 - k: type-2 bit 60 + k
    // the 80 bits four places up (bit s + 4 = type-2 bit s: the CRC bits fill the high word from bit 0), so
    // that the 5-bit window of a step -- its own bit and the four before it -- starts at bit `step`
    const uint64_t vlo = t1 << 4, vhi = rev;
    uint32_t acc = 0;   // WERR | WSUM << 16 (each at most 120 x 128 < 2^16)
#pragma unroll
    for (int u = 0; u < 2; ++u) {   // type-5 position lane + 64 u (s is 0 past the 120)
        const int step = k.step[u];
        const uint32_t win = step < 64 ? (uint32_t)(vlo >> step) | (step ? (uint32_t)(vhi << (64 - step)) : 0u)
                                       : (uint32_t)(vhi >> (step - 64));
        const uint32_t c = ((uint32_t)__popc(win & k.taps[u]) ^ k.scr[u]) & 1u;
        const uint32_t mag = (uint32_t)(s[u] < 0 ? -s[u] : s[u]);
        const bool bad = s[u] != 0 && (uint32_t)(s[u] < 0) != c;
        acc += (bad ? mag : 0u) | (mag << 16);
    }
    acc = wave_sum(acc);
    return max(1, (int32_t)(acc >> 16) - 2 * (int32_t)(acc & 0xFFFFu));
}

// One WAVE per group of G <= VOTE_MAXG rows, after the BSCH blocks of every row are decoded.
__global__ __launch_bounds__(64 * VOTE_WAVES) void k_cell_vote_groups(
    int NG, int G, const int8_t *__restrict__ softbits, long row_bits, int origin, const int32_t *__restrict__ nburst,
    const int32_t *__restrict__ bursts, const int32_t *__restrict__ blocks, const uint8_t *__restrict__ type1,
    uint32_t *__restrict__ cell_init /*[NG]*/, int32_t *__restrict__ score /*[NG]*/, int cap,
    int32_t *__restrict__ ngood /*[NG] or null*/, int32_t *__restrict__ agree /*[NG] or null*/,
    uint32_t *__restrict__ tab_init /*[NG G]*/, uint8_t *__restrict__ cell_scr) {
    __shared__ uint32_t bal_c[VOTE_WAVES][VOTE_MAXBAL];   // the ballots of a wave's group, in order: init,
    __shared__ int32_t bal_w[VOTE_WAVES][VOTE_MAXBAL];    // weight
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = blockIdx.x * VOTE_WAVES + wv;
    if (g >= NG) return;   // the whole wave (no workgroup barrier below)
    uint32_t *bc = bal_c[wv];
    int32_t *bw = bal_w[wv];
    const size_t row0 = (size_t)g * G;
    // block slot of burst b of a row: the sync kernel's numbering (1 per NDB(n), 2 per NDB(p) / SB)
    auto slot_of = [&](size_t ch, int b) {
        int q = 0;
        for (int p = 0; p < b; ++p) q += bursts[(ch * ETSI_MAXB + p) * 2 + 1] == 0 ? 1 : 2;
        return q;
    };
    const LaneTab tab = lane_tab(lane);
    int n = 0;   // wave-uniform: ballots so far
    for (int i0 = 0; i0 < ETSI_MAXB * G; i0 += 64) {
        const int i = i0 + lane, r = i / ETSI_MAXB, b = i % ETSI_MAXB;
        bool ok = false;
        int q = 0, start = 0;   // of the lane's burst: its block slot and start bit, handed to the wave below
        if (r < G) {
            const size_t ch = row0 + r;
            if (b < min(nburst[ch], ETSI_MAXB) && bursts[(ch * ETSI_MAXB + b) * 2 + 1] == 2) {
                start = bursts[(ch * ETSI_MAXB + b) * 2];
                q = slot_of(ch, b);
                ok = q < ETSI_MAXJ && blocks[(ch * ETSI_MAXJ + q) * 4 + 1] != 0;
            }
        }
        unsigned long long bal = __ballot(ok);
        while (bal && n < VOTE_MAXBAL) {   // the step's good blocks in ballot order, the whole wave on each
            const int src = __ffsll((long long)bal) - 1;
            bal &= bal - 1;
            const size_t ch = row0 + (i0 + src) / ETSI_MAXB;
            const int qq = __builtin_amdgcn_readlane(q, src);
            const uint8_t *t = type1 + (ch * ETSI_MAXJ + qq) * 268;
            const long p0 = (long)origin + __builtin_amdgcn_readlane(start, src) + 94;
            // the init: lanes 0..5 read colour code bit j = type-1 bit 9 - j; lanes 8..31 bit j - 8 of
            // MCC(10) MNC(14), type-1 bit 62 - j (the fields are MSB first)
            const bool use = lane < 6 || (lane >= 8 && lane < 32);
            const uint32_t fb = use ? t[lane < 6 ? 9 - lane : 62 - lane] & 1u : 0u;
            const int32_t w = bsch_weight(t, softbits + ch * (size_t)row_bits, p0, row_bits, lane, tab);
            const unsigned long long f = __ballot(fb != 0);
            const uint32_t ecc = (uint32_t)f & 0x3Fu, mm = (uint32_t)(f >> 8) & 0xFFFFFFu;
            if (lane == 0) {
                bc[n] = (((mm << 6) | ecc) << 2) | 3u;
                bw[n] = w;
            }
            ++n;
        }
    }
    // the list is the wave's own: wave-scope ordering is enough
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    const uint32_t inc = cell_init[g];
    uint32_t win = inc;
    if (n > 0) {
        // total | count << 23 of the ballots for init c (every ballot with all = true)
        auto tally = [&](uint32_t c, bool all) {
            uint32_t v = 0;
            for (int k = lane; k < n; k += 64)
                if (all || bc[k] == c) v += (uint32_t)bw[k] + (1u << 23);
            return wave_sum(v);
        };
        const long S = max(score[g], 0);
        const long total = S + (long)(tally(0, true) & 0x7FFFFFu);   // every candidate's T together
        uint32_t v = tally(inc, false);
        long bestT = S + (long)(v & 0x7FFFFFu);
        int nagree = (int)(v >> 23);
        // a challenger takes over with a larger total; among challengers a tie goes to the later ballot
        for (int j = 0; j < n; ++j) {
            const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)bc[j]);
            if (c == inc || c == win) continue;   // (its total is known)
            v = tally(c, false);
            const long T = (long)(v & 0x7FFFFFu);
            if (T > bestT || (win != inc && T == bestT)) {
                win = c;
                bestT = T;
                nagree = (int)(v >> 23);
            }
        }
        if (lane == 0) {
            cell_init[g] = win;
            const long d = 2 * bestT - total;   // T(winner) - the others' totals
            score[g] = (int32_t)(d < 1 ? 1 : d > cap ? cap : d);
            if (agree) agree[g] = nagree;
        }
    } else if (lane == 0 && agree) {
        agree[g] = 0;
    }
    if (lane == 0 && ngood) ngood[g] = n;

    // the winner's scrambler sequence, formed once (SCR_MASK, a lane's dwords w = lane and lane + 64) and
    // stored as whole dwords to the 432-byte table row of every row of the group whose tab_init differs
    uint32_t v0 = 0, v1 = 0;
    bool have = false;
    for (int r0 = 0; r0 < G; r0 += 64) {
        const int r = r0 + lane;
        const bool need = r < G && tab_init[row0 + r] != win;
        unsigned long long m = __ballot(need);
        if (m && !have) {
            auto dword = [&](int w) {
                const uint4 k = *reinterpret_cast<const uint4 *>(&SCR_MASK.w[4 * w]);
                return ((uint32_t)__popc(win & k.x) & 1u) | (((uint32_t)__popc(win & k.y) & 1u) << 8) |
                       (((uint32_t)__popc(win & k.z) & 1u) << 16) | (((uint32_t)__popc(win & k.w) & 1u) << 24);
            };
            v0 = dword(lane);
            v1 = dword(min(lane + 64, 107));
            have = true;
        }
        if (need) tab_init[row0 + r] = win;
        while (m) {   // wave-uniform: one coalesced 432-byte store per row
            const int rr = r0 + __ffsll((long long)m) - 1;
            m &= m - 1;
            uint32_t *o = reinterpret_cast<uint32_t *>(cell_scr + (row0 + rr) * 432);
            o[lane] = v0;
            if (lane < 44) o[64 + lane] = v1;
        }
    }
}

}  // namespace

void launch_cell_vote(tetra_ctx *ctx, size_t NG, size_t G, const int8_t *softbits, size_t row_bits, int origin,
                      const int32_t *nburst, const int32_t *bursts, const int32_t *blocks, const uint8_t *type1,
                      uint32_t *cell_init, int32_t *score, int32_t cap, int32_t *ngood, int32_t *agree,
                      uint32_t *tab_init, uint8_t *cell_scr) {
    hipLaunchKernelGGL(k_cell_vote_groups, dim3(grid_for(NG, VOTE_WAVES)), dim3(64 * VOTE_WAVES), 0, ctx->stream, (int)NG,
                       (int)G, softbits, (long)row_bits, origin, nburst, bursts, blocks, type1, cell_init, score, (int)cap,
                       ngood, agree, tab_init, cell_scr);
}
