// etsi_lock.hip -- loss-of-lock monitor of the streaming ETSI demod on gfx950 (tetra_etsi_lock): a
// post-pass over the soft bits tetra_demod_etsi_stream wrote and the track it left, restated in
// tests/_etsi_lock_model.py.
//
//   k_etsi_lock  one wave per channel, four channels per 256-thread workgroup.  A lane takes 16 B (8
//               dibits) of the row a step from the first 16-B boundary on; the up to 7 dibits in front
//               of it and the up to 7 behind the last whole vector go one to a lane as 2-B loads (a row
//               at an odd address has no aligned dibit: it is read in 2-B pieces throughout).  The byte
//               work stays packed: |s| of four bytes in one dword, then the two bytes of a dibit as
//               the halves of two 16-bit pairs -- packed max / min, the weak compare as a carry into
//               bit 15 -- and three integer sums per lane, reduced over the wave with shuffles.  Lane 0
//               applies the rule and writes the record, the state and track.acquired.  No LDS, no
//               barrier; a wave past the last channel ends at once.
#include "common.h"

namespace {

constexpr int LK_WAVE = 64, LK_ROWS = 4, LK_BLOCK = LK_WAVE * LK_ROWS;
static_assert(TETRA_LOCK_FIELDS == 8 && sizeof(tetra_etsi_lock_state) == 32 && sizeof(tetra_etsi_track) == 32,
              "record layout");

typedef unsigned short lk_u16x2 __attribute__((ext_vector_type(2)));

struct LkSums {
    uint32_t smin = 0, smax = 0, strong = 0;
};

// |s| of four int8 in one dword, as unsigned bytes (-128 -> 128).  A negative byte is complemented and
// incremented: its complement is at most 0x7F, so no carry leaves a byte.
__device__ __forceinline__ uint32_t abs4(uint32_t v) {
    const uint32_t m = (v >> 7) & 0x01010101u;
    return (v ^ (m * 0xFFu)) + m;
}

// Two dibits (s0, s1, s0, s1 in ascending bytes) of |s| bytes; wk = 0x8000 - weak in both halves, weak
// clamped to 0 .. 129.  Adds lo, hi and 1 of every strong dibit to the packed accumulators.
__device__ __forceinline__ void two_dibits(uint32_t a, uint32_t wk, uint32_t &lo_acc, uint32_t &hi_acc, uint32_t &cnt) {
    const uint32_t x = a & 0x00FF00FFu, y = (a >> 8) & 0x00FF00FFu;   // |s0|, |s1| as 16-bit pairs
    const lk_u16x2 xv = __builtin_bit_cast(lk_u16x2, x), yv = __builtin_bit_cast(lk_u16x2, y);
    const uint32_t hi = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(xv, yv));
    const uint32_t lo = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(xv, yv));
    // hi <= 128 and 0x8000 - weak >= 0x7F7F: bit 15 of a half is set iff hi >= weak, nothing carries over
    const uint32_t st = ((hi + wk) >> 15) & 0x00010001u;
    const uint32_t mask = st * 0xFFFFu;
    lo_acc += lo & mask;   // a half grows by at most 128 a call: the callers unpack after at most 4
    hi_acc += hi & mask;
    cnt += st;
}

__device__ __forceinline__ void unpack(LkSums &s, uint32_t lo_acc, uint32_t hi_acc, uint32_t cnt) {
    s.smin += (lo_acc & 0xFFFFu) + (lo_acc >> 16);
    s.smax += (hi_acc & 0xFFFFu) + (hi_acc >> 16);
    s.strong += (cnt & 0xFFFFu) + (cnt >> 16);
}

__device__ __forceinline__ void one_dibit(LkSums &s, const int8_t *p, uint32_t wk) {
    // the second dibit of the dword is zero: with weak >= 1 it is weak and adds nothing; with weak <= 0 it
    // would count as strong, so only the low half's count is taken
    const uint32_t v = (uint32_t)(uint8_t)p[0] | ((uint32_t)(uint8_t)p[1] << 8);
    uint32_t lo = 0, hi = 0, cnt = 0;
    two_dibits(abs4(v), wk, lo, hi, cnt);
    s.smin += lo & 0xFFFFu;
    s.smax += hi & 0xFFFFu;
    s.strong += cnt & 0xFFFFu;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int m = LK_WAVE / 2; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, LK_WAVE);
    return v;
}

__global__ __launch_bounds__(LK_BLOCK) void k_etsi_lock(const int8_t *__restrict__ softbits,
                                                        const int32_t *__restrict__ nsym, int C, long ostride,
                                                        int num, int den, int weak, int nmin, int patience,
                                                        tetra_etsi_track *__restrict__ track,
                                                        tetra_etsi_lock_state *__restrict__ state,
                                                        int32_t *__restrict__ rec) {
    const int lane = threadIdx.x % LK_WAVE;
    const long ch = (long)blockIdx.x * LK_ROWS + threadIdx.x / LK_WAVE;   // wave-uniform
    if (ch >= C) return;
    const int8_t *row = softbits + ch * 2 * ostride;
    const long N = min(max((long)nsym[ch] - 1, 0L), ostride);
    const uint32_t wk = 0x8000u - (uint32_t)min(max(weak, 0), 129);
    const uint32_t wk2 = wk | (wk << 16);

    LkSums s;
    const uintptr_t addr = (uintptr_t)row;
    // dibits in front of the first 16-B boundary (all of them when the row sits at an odd address)
    const long head = (addr & 1) ? N : min((long)((0 - addr) & 15) / 2, N);
    for (long i = lane; i < head; i += LK_WAVE) one_dibit(s, row + 2 * i, wk2);
    const long nvec = (N - head) / 8;
    const uint4 *vp = reinterpret_cast<const uint4 *>(row + 2 * head);   // 16-B aligned when nvec > 0
    for (long v = lane; v < nvec; v += LK_WAVE) {
        const uint4 q = vp[v];   // bytes 2 head + 16 v .. + 15 <= 2 N - 1
        uint32_t lo = 0, hi = 0, cnt = 0;
        two_dibits(abs4(q.x), wk2, lo, hi, cnt);
        two_dibits(abs4(q.y), wk2, lo, hi, cnt);
        two_dibits(abs4(q.z), wk2, lo, hi, cnt);
        two_dibits(abs4(q.w), wk2, lo, hi, cnt);
        unpack(s, lo, hi, cnt);
    }
    for (long i = head + 8 * nvec + lane; i < N; i += LK_WAVE) one_dibit(s, row + 2 * i, wk2);   // fewer than 8 left

    const uint32_t smin = wave_sum(s.smin), smax = wave_sum(s.smax), strong = wave_sum(s.strong);
    if (lane != 0) return;

    tetra_etsi_lock_state st = state[ch];
    if ((st.searching | st.bad_run | st.relocks | st.chunks) == 0) st.searching = 1;   // a new stream acquires
    const bool fresh = st.searching != 0;
    const bool railed = fabsf(track[ch].delta) >= 1.5f;
    const bool judged = N >= (long)nmin;
    const long nweak = N - (long)strong;
    const bool bad = judged && (2 * nweak > N || smax == 0 || (int64_t)smin * den < (int64_t)num * smax || railed);
    bool dropped = false, clear = false;
    st.chunks += 1;
    if (judged && !bad) {
        st.searching = 0;
        st.bad_run = 0;
    } else if (judged && fresh) {
        st.searching = 1;
        clear = true;
    } else if (judged) {
        st.bad_run += 1;
        if (st.bad_run >= patience) {
            dropped = clear = true;
            st.searching = 1;
            st.bad_run = 0;
            st.relocks += 1;
        }
    }
    state[ch].searching = st.searching;
    state[ch].bad_run = st.bad_run;
    state[ch].relocks = st.relocks;
    state[ch].chunks = st.chunks;
    if (clear) track[ch].acquired = 0;
    int32_t *o = rec + ch * TETRA_LOCK_FIELDS;
    o[TETRA_LOCK_SMIN] = (int32_t)smin;
    o[TETRA_LOCK_SMAX] = (int32_t)smax;
    o[TETRA_LOCK_N] = (int32_t)N;
    o[TETRA_LOCK_WEAK] = (int32_t)nweak;
    o[TETRA_LOCK_FLAGS] = (judged ? TETRA_LOCK_JUDGED : 0) | (bad ? TETRA_LOCK_BAD : 0) | (railed ? TETRA_LOCK_RAILED : 0) |
                          (fresh ? TETRA_LOCK_FRESH : 0) | (dropped ? TETRA_LOCK_DROPPED : 0) |
                          (st.searching ? TETRA_LOCK_SEARCHING : 0);
    o[TETRA_LOCK_BAD_RUN] = st.bad_run;
    o[TETRA_LOCK_RELOCKS] = st.relocks;
    o[7] = 0;
}

}  // namespace

extern "C" int tetra_etsi_lock(tetra_ctx *ctx, const int8_t *softbits, const int32_t *nsym, size_t C, size_t ostride,
                               int32_t num, int32_t den, int32_t weak, int32_t nmin, int32_t patience,
                               tetra_etsi_track *track, tetra_etsi_lock_state *state, int32_t *rec) {
    if (!ctx) return TETRA_E_INVALID;
    if (C == 0 || ostride == 0 || !softbits || !nsym || !track || !state || !rec)
        return tetra_fail(ctx, TETRA_E_INVALID, "tetra_etsi_lock: C > 0, ostride > 0 and every array");
    if (den <= 0 || num < 0 || patience < 1)
        return tetra_fail(ctx, TETRA_E_INVALID, "tetra_etsi_lock: num >= 0, den > 0, patience >= 1 (num %d, den %d, "
                          "patience %d)", (int)num, (int)den, (int)patience);
    if (C > ((size_t)1 << 24) || ostride > ((size_t)1 << 23))
        return tetra_fail(ctx, TETRA_E_INVALID, "too many rows or too long a row for one tetra_etsi_lock call");
    Staging st(ctx);
    const int8_t *sb = (const int8_t *)st.in(softbits, C * ostride * 2);
    const int32_t *ns = (const int32_t *)st.in(nsym, C * 4);
    tetra_etsi_track *tr = (tetra_etsi_track *)st.inout(track, C * sizeof(tetra_etsi_track));
    tetra_etsi_lock_state *ls = (tetra_etsi_lock_state *)st.inout(state, C * sizeof(tetra_etsi_lock_state));
    int32_t *ro = (int32_t *)st.out(rec, C * TETRA_LOCK_FIELDS * 4);
    if (!sb || !ns || !tr || !ls || !ro) return st.finish();
    {
        PROF(ctx, "etsi_lock");
        hipLaunchKernelGGL(k_etsi_lock, dim3(grid_for(C, LK_ROWS)), dim3(LK_BLOCK), 0, ctx->stream, sb, ns, (int)C,
                           (long)ostride, (int)num, (int)den, (int)weak, (int)nmin, (int)patience, tr, ls, ro);
    }
    return st.finish();
}
