// etsi_chanfilt_r.hip -- the ETSI channel filter, one stream per wave: the north-star chain's first and
// largest kernel.
//
//   k_chanfilt_r stage 1: 48-tap decimate-by-10 FIR (2.4 MSps -> 240 kHz), stage 2: polyphase RRC
//                (alpha 0.35, 321 taps at 720 kHz) resampler x3/10 -> 72 kHz = 4 samples/symbol,
//                then the timing stage (fused).  cf32 (8 B/sample) and SC16 (4 B/sample) chunks up
//                to YLDS outputs: the workgroup's four waves stream the channel's quarters
//                independently (480-sample wave tiles, register prefetch, private LDS image and
//                stage-1 buffer; stage 1 in registers: a lane's 10-sample block from the image, the
//                next four blocks from its row neighbours by DPP folded into v_fmac_f32_dpp; stage 2
//                in one-MFMA-tile bursts on v_mfma_f32_16x16x4_f32 -- exact f32: banded tap matrix x
//                16 columns of 5 output triples), y held in LDS.
#include "etsi_chanfilt.h"

namespace {

// --------------------------------------------------------------------------- per-wave channel filter
// cf32 and SC16 with y in LDS (M2 <= YLDS): the workgroup's waves stream the channel's quarters
// independently.  Wave w owns the stage-2 triples [U_w, U_w+1) and the stage-1 outputs
// [K_w, K_w+1), K_w = 10 U_w (the last wave's end is M1), in wave tiles with its own LDS image and
// stage-1 buffer, and runs a one-MFMA-tile stage-2 burst (40 triples: one dependent chain of 39
// MFMAs) whenever 40 triples have their windows.  So the stream has no workgroup barrier until the
// channel ends, and a burst stalls one wave's quarter of the loads in flight instead of the whole
// workgroup's (k_chanfilt: every wave waits at the tile's barriers while three of them run the
// burst's MFMA pairs).  Wave w's last triples need stage-1 outputs up to K_w+1 + 103, the first
// ones of wave w + 1, which that wave also copies into a seam buffer.  A wave bursts every ready
// triple at its last tile, so after the one barrier at the channel's end it appends its seam and
// runs one burst of the <= 12 triples left, then the timing tail as in k_chanfilt.  Every output is
// the same fma chain as in k_chanfilt (bit-identical to the oracle).  (Round 3 ran cf32 on
// k_chanfilt_w, the same structure with each lane reading its whole 48-sample window and the taps
// from LDS; k_chanfilt_r below replaced it)
constexpr int WLR = 568;                    // wave stage-1 buffer (float2): < 567 entries in the stream,
                                            // <= 265 in the channel's last (seam) burst
constexpr int SEAM = 112;                   // >= the 104 outputs a left neighbour's last triples need
constexpr int UMIN = 16;                    // triples per wave at least (10 UMIN >= SEAM)
static_assert(sizeof(TrackOut) + sizeof(int) <= 48 && (4 * WLR + 3 * SEAM) % 2 == 0, "per-wave demod LDS carving");

// cross-lane LDS hand-off inside one wave: a wave's LDS instructions execute in order, so only the
// compiler has to be kept from moving accesses across this point (no s_waitcnt, no s_barrier)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// --------------------------------------------------------------------------- register stage 1
// k_chanfilt_r: the per-wave channel filter with stage 1 out of LDS.  With each lane reading its
// whole 48-sample window (24 float4) and the 48 taps (12 broadcast float4) from LDS for one output
// (round 3's k_chanfilt_w), stage 1 costs ~5 LDS cycles per output of the CU's 128 B/cycle, and
// that bounds the filter once the input needs no HBM (timing builds, input L2-resident: 0.93 ms per
// 8192 x 131072 batch without the tail; with stage 1's chain cut to a third, 0.66).  Here a lane reads
// only its own 10-sample block from the image (5 loads of 2 samples) and takes the next four blocks
// from its row neighbours with DPP (row_shl:p reads lane + p of the same 16-lane row): a row of 16
// lanes holds 16 consecutive blocks and computes the outputs of its first 12, so a wave tile is 48
// outputs (480 new samples, a 40-sample halo).  The taps sit in registers.  Each output is still the
// oracle's ascending-j fma chain (x[10 k + j] is sample j mod 10 of lane + j / 10's block),
// bit-identical.  SC16 keeps its samples as raw dwords in the image (re low 16 bits, im high) and
// folds the 2^-15 scale into the taps (an exact power of two: fma(h 2^-15, x, a) == fma(h, x 2^-15, a)).
constexpr int RHALO = 40;           // image samples carried over from the previous tile
template <typename In> struct RCfg;
// nb: 10-sample blocks per lane.  nb = 1: a row's 16 lanes hold 16 blocks and compute the outputs
// of the first 12 (DPP shifts of 1..4 lanes); nb = 2: lane i holds blocks 2i, 2i + 1, a row 32
// blocks, outputs of the first 28 (shifts of 1..2 lanes) -- 14 of 16 lanes' work kept instead of 12
// and the per-tile work (loads, image, halo, burst test) spread over 112 outputs instead of 48.
// cf32 keeps nb = 1: its 9.3 KB nb = 2 image would not fit two workgroups per CU.
// pf: input tiles in flight per wave (register prefetch).
template <> struct RCfg<uint4> { static constexpr int bps = 4, pf = 2, nb = 2, wlr = 632; };   // SC16: 16-B load = 4 samples
template <> struct RCfg<float4> { static constexpr int bps = 8, pf = 3, nb = 1, wlr = WLR; };  // cf32: 2 samples (4 tiles: spills)
template <typename In> constexpr int r_tk() { return RCfg<In>::nb == 1 ? 48 : 112; }   // stage-1 outputs per wave tile
template <typename In> constexpr int r_chunks() { return 10 * r_tk<In>() * RCfg<In>::bps / 16; }   // 16-B loads per tile
// per-wave image: two halo slots (tile t reads slot t & 1; tile t's last RHALO samples are also
// written into slot (t + 1) & 1 as they arrive, so no halo copy) + the tile's 10 TK samples
template <typename In> constexpr int r_img16() { return (2 * RHALO + 10 * r_tk<In>()) * RCfg<In>::bps / 16; }
template <typename In> constexpr int r_smem4() {
    return 3 + 4 * r_img16<In>() + (4 * RCfg<In>::wlr + 3 * SEAM + YLDS) / 2;
}
// tail staging over the freed images + stage-1 buffers: d_j, soft bits, hard dibits, O-M parts, symbols
constexpr int r_tail_bytes() { return 19 * WTAIL_SM + 48 + 1024; }
static_assert(r_tail_bytes() <= 4 * r_img16<float4>() * 16 + 4 * WLR * 8, "k_chanfilt_r tail staging");
// two workgroups per CU with >= 9.5 KB of the CU's LDS left for the lower MAC's kernels
// (k_etsi_viterbi 7 KB, k_etsi_sync 2.4 KB), which the bench's pipeline runs beside the next demod
static_assert(2 * r_smem4<float4>() * 16 + 7 * 1024 + 2560 <= 160 * 1024, "k_chanfilt_r LDS (cf32)");
static_assert(2 * r_smem4<uint4>() * 16 + 7 * 1024 + 2560 <= 160 * 1024, "k_chanfilt_r LDS (SC16)");
// a stage-1 buffer holds < 10 x 39 + 123 + one tile's outputs (the burst test runs once per tile)
static_assert(RCfg<uint4>::wlr >= 513 + 112 && WLR >= 513 + 48, "stage-1 buffer");

// ar += h[q] * x_re[q], ai += h[q] * x_im[q] for q < N in order, x taken from lane + P of this
// lane's 16-lane row (row_shl:P; a lane past the row's end reads 0 -- only lanes whose outputs are
// not kept do): one v_fmac_f32_dpp per product, the DPP folded into the fma (hipcc emits a
// v_mov_b32_dpp per operand instead and keeps ~76 of them live).  Five products per asm: the hazard
// recognizer puts a wait state after every asm statement.  A DPP read needs two wait states after
// the VALU write of its source: where the chain's order does not already put this lane's own use
// of x (and so its conversion) >= 9 steps earlier, NOP = true opens the block with s_nop 1.
template <int P, int N, bool NOP = false>
__device__ __forceinline__ void fmac_rows(float &ar, float &ai, const float *xr, const float *xi, const float *h) {
    if constexpr (P == 0) {   // in-lane: one v_pk_fma_f32 per product (both halves' fma, the same bits)
        pf2 a = {ar, ai};
#pragma unroll
        for (int q = 0; q < N; ++q) a = pfma(h[q], pf2{xr[q], xi[q]}, a);
        ar = a.x;
        ai = a.y;
    }
    else if constexpr (P == 1 && N == 5 && !NOP) {
        asm("v_fmac_f32_dpp %0, %2, %12 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %12 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %13 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %8, %13 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %14 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %9, %14 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %5, %15 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %10, %15 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %6, %16 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %11, %16 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xr[3]), "v"(xr[4]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(xi[3]), "v"(xi[4]), "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]), "v"(h[4]));
    }
    else if constexpr (P == 1 && N == 5 && NOP) {
        asm("s_nop 1\n\t"
            "v_fmac_f32_dpp %0, %2, %12 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %12 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %13 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %8, %13 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %14 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %9, %14 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %5, %15 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %10, %15 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %6, %16 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %11, %16 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xr[3]), "v"(xr[4]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(xi[3]), "v"(xi[4]), "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]), "v"(h[4]));
    }
    else if constexpr (P == 1 && N == 3 && !NOP) {
        asm("v_fmac_f32_dpp %0, %2, %8 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %5, %8 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %9 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %6, %9 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %10 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %10 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(h[0]), "v"(h[1]), "v"(h[2]));
    }
    else if constexpr (P == 1 && N == 3 && NOP) {
        asm("s_nop 1\n\t"
            "v_fmac_f32_dpp %0, %2, %8 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %5, %8 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %9 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %6, %9 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %10 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %10 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(h[0]), "v"(h[1]), "v"(h[2]));
    }
    else if constexpr (P == 2 && N == 5 && !NOP) {
        asm("v_fmac_f32_dpp %0, %2, %12 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %12 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %13 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %8, %13 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %14 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %9, %14 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %5, %15 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %10, %15 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %6, %16 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %11, %16 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xr[3]), "v"(xr[4]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(xi[3]), "v"(xi[4]), "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]), "v"(h[4]));
    }
    else if constexpr (P == 2 && N == 5 && NOP) {
        asm("s_nop 1\n\t"
            "v_fmac_f32_dpp %0, %2, %12 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %12 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %13 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %8, %13 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %14 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %9, %14 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %5, %15 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %10, %15 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %6, %16 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %11, %16 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xr[3]), "v"(xr[4]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(xi[3]), "v"(xi[4]), "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]), "v"(h[4]));
    }
    else if constexpr (P == 2 && N == 3 && !NOP) {
        asm("v_fmac_f32_dpp %0, %2, %8 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %5, %8 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %9 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %6, %9 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %10 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %10 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(h[0]), "v"(h[1]), "v"(h[2]));
    }
    else if constexpr (P == 2 && N == 3 && NOP) {
        asm("s_nop 1\n\t"
            "v_fmac_f32_dpp %0, %2, %8 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %5, %8 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %9 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %6, %9 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %10 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %10 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(h[0]), "v"(h[1]), "v"(h[2]));
    }
    else if constexpr (P == 3 && N == 5 && !NOP) {
        asm("v_fmac_f32_dpp %0, %2, %12 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %12 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %13 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %8, %13 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %14 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %9, %14 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %5, %15 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %10, %15 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %6, %16 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %11, %16 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xr[3]), "v"(xr[4]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(xi[3]), "v"(xi[4]), "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]), "v"(h[4]));
    }
    else if constexpr (P == 3 && N == 5 && NOP) {
        asm("s_nop 1\n\t"
            "v_fmac_f32_dpp %0, %2, %12 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %12 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %13 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %8, %13 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %14 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %9, %14 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %5, %15 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %10, %15 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %6, %16 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %11, %16 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xr[3]), "v"(xr[4]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(xi[3]), "v"(xi[4]), "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]), "v"(h[4]));
    }
    else if constexpr (P == 3 && N == 3 && !NOP) {
        asm("v_fmac_f32_dpp %0, %2, %8 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %5, %8 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %9 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %6, %9 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %10 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %10 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(h[0]), "v"(h[1]), "v"(h[2]));
    }
    else if constexpr (P == 3 && N == 3 && NOP) {
        asm("s_nop 1\n\t"
            "v_fmac_f32_dpp %0, %2, %8 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %5, %8 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %9 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %6, %9 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %10 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %10 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(h[0]), "v"(h[1]), "v"(h[2]));
    }
    else if constexpr (P == 4 && N == 5 && !NOP) {
        asm("v_fmac_f32_dpp %0, %2, %12 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %12 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %13 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %8, %13 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %14 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %9, %14 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %5, %15 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %10, %15 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %6, %16 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %11, %16 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xr[3]), "v"(xr[4]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(xi[3]), "v"(xi[4]), "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]), "v"(h[4]));
    }
    else if constexpr (P == 4 && N == 5 && NOP) {
        asm("s_nop 1\n\t"
            "v_fmac_f32_dpp %0, %2, %12 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %12 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %13 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %8, %13 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %14 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %9, %14 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %5, %15 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %10, %15 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %6, %16 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %11, %16 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xr[3]), "v"(xr[4]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(xi[3]), "v"(xi[4]), "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]), "v"(h[4]));
    }
    else if constexpr (P == 4 && N == 3 && !NOP) {
        asm("v_fmac_f32_dpp %0, %2, %8 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %5, %8 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %9 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %6, %9 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %10 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %10 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(h[0]), "v"(h[1]), "v"(h[2]));
    }
    else if constexpr (P == 4 && N == 3 && NOP) {
        asm("s_nop 1\n\t"
            "v_fmac_f32_dpp %0, %2, %8 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %5, %8 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %3, %9 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %6, %9 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %0, %4, %10 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_fmac_f32_dpp %1, %7, %10 row_shl:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            : "+v"(ar), "+v"(ai)
            : "v"(xr[0]), "v"(xr[1]), "v"(xr[2]), "v"(xi[0]), "v"(xi[1]), "v"(xi[2]), "v"(h[0]), "v"(h[1]), "v"(h[2]));
    }
    else {
        static_assert(P == 0, "fmac_rows: no such form");
    }
}

// (Round 4 measured and removed a form with y in a global scratch, one tile prefetched and three
// workgroups per CU for SC16: 0.938 -> 1.05 ms)
template <typename In, bool FUSE>
__global__ __launch_bounds__(256, 2) void k_chanfilt_r(const In *__restrict__ iq, long N, int M1, int M2,
                                                       const float *__restrict__ h1, const float *__restrict__ afrag,
                                                       float2 *__restrict__ y, TimingOut to, long ld) {
    constexpr bool SC16 = std::is_same<In, uint4>::value;
    constexpr int BPS = RCfg<In>::bps, PF = RCfg<In>::pf, NCH = r_chunks<In>(), NL = (NCH + 63) / 64;
    constexpr int NB = RCfg<In>::nb, TK = r_tk<In>(), TIN = 10 * TK, LR = RCfg<In>::wlr;
    constexpr int ROWK = NB == 1 ? 12 : 28;    // outputs per 16-lane row
    constexpr int RH16 = RHALO * BPS / 16;     // 16-B chunks per halo
    constexpr int IMGB = r_img16<In>() * 16;   // image bytes per wave
    using Pair = typename std::conditional<SC16, uint2, float4>::type;   // two samples
    __shared__ float4 smem[r_smem4<In>()];
    TrackOut *tro = reinterpret_cast<TrackOut *>(smem);                        // + prog: 3 float4
    uint8_t *img_all = reinterpret_cast<uint8_t *>(smem + 3);                  // 4 wave images
    float2 *lin_all = reinterpret_cast<float2 *>(img_all + 4 * IMGB);          // 4 stage-1 buffers
    float2 *seam = lin_all + 4 * LR;
    const int ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const uint32_t t_start = FUSE && to.probe && tid == 0 ? (uint32_t)wall_clock64() : 0u;
    float *yb = reinterpret_cast<float *>(seam + 3 * SEAM);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint8_t *img = img_all + wv * IMGB;
    float2 *lin = lin_all + wv * LR;
    for (int i = lane; i < LR; i += 64) lin[i] = make_float2(0.f, 0.f);
    float at[S2K];
#pragma unroll
    for (int k = 0; k < S2K; ++k) at[k] = afrag[64 * k + lane];
    // SC16: the launch passes the taps pre-scaled by 2^-15.  Taps 10..47 are v_fmac_f32_dpp's src1 and
    // must be VGPRs (left as SGPRs hipcc copies them into VGPRs every tile); taps 0..9 (the in-lane
    // products) stay scalar operands
    float hv[48];
#pragma unroll
    for (int j = 0; j < 48; ++j) {
        hv[j] = h1[j];
        if (j >= 10) asm volatile("" : "+v"(hv[j]));
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): landed before the stream starts
    // the partition
    const int UT = (M2 + 2) / 3;
    const int nw = min(4, max(1, UT / UMIN));
    const int UQ = (UT + nw - 1) / nw;
    const bool active = wv < nw;
    const bool has_right = wv + 1 < nw;
    const int u_beg = min(wv * UQ, UT), u_end = has_right ? (wv + 1) * UQ : UT;
    const int K0 = 10 * u_beg, K1 = has_right ? 10 * u_end : M1;
    const int ntile = active ? (K1 - K0 + 4 + TK - 1) / TK : 0;   // wave tiles with kfirst < K1
    // tile t: lane (row ro, i) holds the NB blocks of x240[K0 + TK t - 4 + ROWK ro + NB i + e], e < NB,
    // samples 10 (K0 + TK t) - 40 + 10 (ROWK ro + NB i + e) + [0, 10) = image samples
    // 10 (ROWK ro + NB i + e) + [0, 10); the tile's new samples 10 (K0 + TK t) + [0, 10 TK) land at
    // image sample 40.  A buffer resource over the wave's samples [10 K0, last needed]: loads past
    // it return 0 without touching memory.
    const long s0 = 10L * K0;
    const long slast = active ? min(10L * (K1 - 1) + 47, N - 1) : s0;
    const uint8_t *xp = reinterpret_cast<const uint8_t *>(iq) + ((size_t)ch * ld + s0) * BPS;   // rows ld apart
    const int nbytes = active ? (int)(((slast - s0 + 1) * BPS + 15) & ~15L) : 0;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(xp), 0, nbytes, 0x00020000);
    const int ro = lane >> 4, li = lane & 15;
    const int blk = ROWK * ro + NB * li;   // this lane's first block
    auto load_tile = [&](In (&pf)[NL], int t) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < NL; ++r) {
            const int c = min(64 * r + lane, NCH - 1);   // unconditional (a branch makes hipcc wait at the join)
            const nt_f4 v = __builtin_amdgcn_raw_buffer_load_b128(xr, 16 * c, t * TIN * BPS, 2 /* nt */);
            pf[r] = *reinterpret_cast<const In *>(&v);
        }
    };
    int kbase = K0;      // x240 index of lin[0]
    int u_done = u_beg;  // triples [u_beg, u_done) are in yb
    const int kg = lane >> 4, seg = (lane & 15) >> 1, comp = lane & 1;
    const float *lf = reinterpret_cast<const float *>(lin);
    // one MFMA tile: triples [u_done, u_done + 40) as 8 segments x 5 (columns = 2 seg + comp), only
    // triples < u_lim stored; a column past u_lim reads the buffer's start (finite, never stored).
    // B operands one 13-step chunk ahead of the MFMAs that use them (hipcc otherwise waits one LDS
    // round trip before every MFMA pair of the dependent chain)
    auto burst = [&](int u_lim) __attribute__((always_inline)) {
        const int U0 = u_done + S2Q * seg;
        const int b0 = U0 < u_lim ? 2 * (10 * U0 - kbase + kg) + comp : 2 * kg + comp;
        float bv[S2K];
        f4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s2 = 0; s2 < 13; ++s2) bv[s2] = lf[b0 + 8 * s2];
#pragma unroll
        for (int s3 = 0; s3 < 3; ++s3) {
            __builtin_amdgcn_sched_barrier(0);
            if (s3 < 2) {
#pragma unroll
                for (int s2 = 13 * s3 + 13; s2 < 13 * s3 + 26; ++s2) bv[s2] = lf[b0 + 8 * s2];
            }
#pragma unroll
            for (int s2 = 13 * s3; s2 < 13 * s3 + 13; ++s2)
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(at[s2], bv[s2], c, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 4 * kg + r, q = i / 3, m = 3 * U0 + i;
            if (i < 15 && U0 + q < u_lim && m < M2) yb[2 * m + comp] = c[r];
        }
    };
    auto tile = [&](int t, In (&pf)[NL]) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < NL; ++r)
            if (64 * r + lane < NCH) *reinterpret_cast<In *>(img + 2 * RHALO * BPS + 16 * (64 * r + lane)) = pf[r];
        // the tile's last RHALO samples: also the next tile's halo slot
#pragma unroll
        for (int r = 0; r < NL; ++r) {
            const int c = 64 * r + lane - (NCH - RH16);
            if (c >= 0 && c < RH16) *reinterpret_cast<In *>(img + ((t + 1) & 1) * RHALO * BPS + 16 * c) = pf[r];
        }
        __builtin_amdgcn_sched_barrier(0);
        load_tile(pf, t + PF);
        wave_sync();
        // this lane's blocks: 10 NB samples as 5 NB pairs; image sample s < RHALO is in halo slot
        // t & 1, the rest at 2 RHALO + (s - RHALO) (a lane's blocks lie on one side: blk < 4 or >= 4)
        const uint8_t *bimg = img + (10 * blk + (blk < 4 ? (t & 1) * RHALO : RHALO)) * BPS;
        float xre[10 * NB], xim[10 * NB];
#pragma unroll
        for (int m = 0; m < 5 * NB; ++m) {
            const Pair v = *reinterpret_cast<const Pair *>(bimg + 2 * m * BPS);
            if constexpr (SC16) {
                xre[2 * m] = (float)(int16_t)(v.x & 0xFFFFu);
                xim[2 * m] = (float)(int16_t)(v.x >> 16);
                xre[2 * m + 1] = (float)(int16_t)(v.y & 0xFFFFu);
                xim[2 * m + 1] = (float)(int16_t)(v.y >> 16);
            } else {
                xre[2 * m] = v.x;
                xim[2 * m] = v.y;
                xre[2 * m + 1] = v.z;
                xim[2 * m + 1] = v.w;
            }
        }
        // x240[k] = sum_j h1[j] x[10 k + j], j ascending: sample j % 10 of block k + j / 10
        const int k = K0 + TK * t - 4 + blk;
        if constexpr (NB == 1) {   // block k + p: lane + p
            float ar = 0.f, ai = 0.f;
            fmac_rows<0, 10>(ar, ai, xre, xim, hv);
            fmac_rows<1, 5>(ar, ai, xre, xim, hv + 10);
            fmac_rows<1, 5>(ar, ai, xre + 5, xim + 5, hv + 15);
            fmac_rows<2, 5>(ar, ai, xre, xim, hv + 20);
            fmac_rows<2, 5>(ar, ai, xre + 5, xim + 5, hv + 25);
            fmac_rows<3, 5>(ar, ai, xre, xim, hv + 30);
            fmac_rows<3, 5>(ar, ai, xre + 5, xim + 5, hv + 35);
            fmac_rows<4, 5>(ar, ai, xre, xim, hv + 40);
            fmac_rows<4, 3>(ar, ai, xre + 5, xim + 5, hv + 45);
            if (li < 12 && k >= K0 && k < K1) {
                lin[k - kbase] = make_float2(ar, ai);
                if (wv > 0 && k - K0 < SEAM) seam[(wv - 1) * SEAM + k - K0] = make_float2(ar, ai);
            }
        } else {   // output A = block k: blocks k, k+1 in-lane, k+2, k+3 lane + 1, k+4 lane + 2;
                   // output B = block k + 1: k+1 in-lane, k+2, k+3 lane + 1, k+4, k+5 lane + 2
            const float *x0r = xre, *x0i = xim, *x1r = xre + 10, *x1i = xim + 10;
            float ar = 0.f, ai = 0.f, br = 0.f, bi = 0.f;
            fmac_rows<0, 10>(ar, ai, x0r, x0i, hv);
            fmac_rows<0, 10>(ar, ai, x1r, x1i, hv + 10);
            fmac_rows<0, 10>(br, bi, x1r, x1i, hv);
            fmac_rows<1, 5, true>(br, bi, x0r, x0i, hv + 10);   // x0's first read in B's chain
            fmac_rows<1, 5>(ar, ai, x0r, x0i, hv + 20);
            fmac_rows<1, 5, true>(br, bi, x0r + 5, x0i + 5, hv + 15);   // and of x0[5..9]
            fmac_rows<1, 5>(ar, ai, x0r + 5, x0i + 5, hv + 25);
            fmac_rows<1, 5>(br, bi, x1r, x1i, hv + 20);
            fmac_rows<1, 5>(ar, ai, x1r, x1i, hv + 30);
            fmac_rows<1, 5>(br, bi, x1r + 5, x1i + 5, hv + 25);
            fmac_rows<1, 5>(ar, ai, x1r + 5, x1i + 5, hv + 35);
            fmac_rows<2, 5>(br, bi, x0r, x0i, hv + 30);
            fmac_rows<2, 5>(ar, ai, x0r, x0i, hv + 40);
            fmac_rows<2, 5>(br, bi, x0r + 5, x0i + 5, hv + 35);
            fmac_rows<2, 3>(ar, ai, x0r + 5, x0i + 5, hv + 45);
            fmac_rows<2, 5>(br, bi, x1r, x1i, hv + 40);
            fmac_rows<2, 3>(br, bi, x1r + 5, x1i + 5, hv + 45);
            if (li < 14) {
                const bool va = k >= K0 && k < K1, vb = k + 1 >= K0 && k + 1 < K1;
                if (va && vb) {   // the two outputs side by side: one 16-B store
                    *reinterpret_cast<float4 *>(lin + (k - kbase)) = make_float4(ar, ai, br, bi);
                } else {
                    if (va) lin[k - kbase] = make_float2(ar, ai);
                    if (vb) lin[k + 1 - kbase] = make_float2(br, bi);
                }
                if (wv > 0) {
                    if (va && k - K0 < SEAM) seam[(wv - 1) * SEAM + k - K0] = make_float2(ar, ai);
                    if (vb && k + 1 - K0 < SEAM) seam[(wv - 1) * SEAM + k + 1 - K0] = make_float2(br, bi);
                }
            }
        }
        wave_sync();
        const int kav = min(K0 + TK * t + TK - 5, K1 - 1);   // the tile's last output
        const int u_rdy = kav >= 113 ? min((kav - 113) / 10 + 1, u_end) : 0;
        while (u_rdy - u_done >= S2T || (t == ntile - 1 && u_rdy > u_done)) {
            const int ul = min(u_done + S2T, u_rdy);
            burst(ul);
            u_done = ul;
            // keep x240[10 u_done, kav] at the buffer's front: <= 10 (one tile's triples) + 123
            const int from = 10 * u_done - kbase, cnt = kav + 1 - 10 * u_done;
            constexpr int NE = (TK + 123 + 63) / 64;
            float2 v[NE];
#pragma unroll
            for (int e = 0; e < NE; ++e) v[e] = lane + 64 * e < cnt ? lin[from + lane + 64 * e] : make_float2(0.f, 0.f);
            wave_sync();
#pragma unroll
            for (int e = 0; e < NE; ++e)
                if (lane + 64 * e < cnt) lin[lane + 64 * e] = v[e];
            kbase = 10 * u_done;
        }
        wave_sync();
    };
    In pf[PF][NL];
    if (ntile > 0) {
#pragma unroll
        for (int u = 0; u < PF; ++u) load_tile(pf[u], u);
    }
    int t = 0;
    for (; t + PF <= ntile; t += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) tile(t + u, pf[u]);
    }
#pragma unroll
    for (int u = 0; u < PF - 1; ++u)
        if (t + u < ntile) tile(t + u, pf[u]);
    __syncthreads();   // every wave's seam and in-loop bursts
    if (active && u_done < u_end) {
        if (has_right) {
            for (int i = lane; i < SEAM; i += 64) lin[K1 - kbase + i] = seam[wv * SEAM + i];
            wave_sync();
        }
        burst(u_end);
    }
    __syncthreads();
    if constexpr (FUSE) {
        // the tail's LDS over the freed images and stage-1 buffers (the launch guarantees
        // sm <= WTAIL_SM): d_j scratch, soft bits, hard dibits, the O-M parts, then the symbols
        const int sm = M2 / 4 + 2;
        uint8_t *R = img_all;
        const int o_sb = (8 * sm + 15) & ~15, o_hd = o_sb + ((2 * sm + 15) & ~15), o_om = o_hd + ((sm + 15) & ~15);
        const TailStage st{reinterpret_cast<float2 *>(R + o_om + 1024), reinterpret_cast<int8_t *>(R + o_sb), R + o_hd};
        int *prog = reinterpret_cast<int *>(tro + 1);
        timing_tail(reinterpret_cast<const float2 *>(yb), reinterpret_cast<float2 *>(R), to, M2, ch, tid, tro, prog,
                    &st, reinterpret_cast<float *>(R + o_om), t_start);
    } else {
        copy_out(reinterpret_cast<uint8_t *>(y + (size_t)ch * M2), reinterpret_cast<const uint8_t *>(yb), 8 * M2, tid);
    }
}

}  // namespace

const void *chanfilt_r_fn(int fmt, bool fused) {
    if (fmt == TETRA_SC16)
        return fused ? reinterpret_cast<const void *>(&k_chanfilt_r<uint4, true>)
                     : reinterpret_cast<const void *>(&k_chanfilt_r<uint4, false>);
    return fused ? reinterpret_cast<const void *>(&k_chanfilt_r<float4, true>)
                 : reinterpret_cast<const void *>(&k_chanfilt_r<float4, false>);
}
