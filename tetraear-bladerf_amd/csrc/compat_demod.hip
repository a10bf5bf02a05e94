// compat_demod.hip -- SignalProcessor.process on gfx950, bit-compatible with the reference: the host
// chain over the three stage units (host code only; the kernels are theirs).
//
// Reference path (/root/reference/tetraear/signal/processor.py:221-273):
//   scipy.signal.decimate(x, q)      cheby1(8,0.05,0.8/q) SOS, sosfiltfilt (odd pad 27)   :254      compat_decimate.hip
//   frequency_shift                   x * exp(-j*2*pi*f*n/fs)                              :85-100   compat_filtfilt.hip
//   filter_signal                     butter(4) + filtfilt (odd pad 15), complex128        :51-83    compat_filtfilt.hip
//   extract_symbols                   best integer phase by mean |x|^2, then gather       :168-219  compat_symbols.hip
//   demodulate_dqpsk                  normalise, differential phase, shifted thresholds   :102-166  compat_symbols.hip
//
// Numerics: every recursion restates the operation order of scipy's compiled loops (no FMA
// contraction: built with -ffp-contract=off), and the vector math follows numpy's kernels on
// x86-64 (complex multiply fma(a,c,-(b*d)) / fma(a,d,b*c); |z| = max*sqrt(fma(r,r,1)),
// pairwise summation for np.mean).  Only sin/cos (mixer) and atan2 (decision) come from a
// different libm, i.e. they can differ from the CPU by an ulp.
//
// Parallel layout: IIR recursions are sequential in time, so one lane owns one real component
// of one channel ("lane = (channel, re|im)"); channels batch across lanes.  Per-lane streams
// live in a "grouped" layout [C/32][time][32 channels][re,im] so the 64 lanes of a wave touch
// 64 consecutive scalars per time step (coalesced).
#include "common.h"
#include "compat_sos.h"   // Lay, the tile limits, the stage entry points

int check_plan(tetra_ctx *ctx, const tetra_compat_plan *P) {
    if (!P) return tetra_fail(ctx, TETRA_E_INVALID, "plan is NULL");
    if (P->sps < 1 || P->phase_step < 1) return tetra_fail(ctx, TETRA_E_INVALID, "bad sps/phase_step");
    return TETRA_OK;
}

namespace {

// Which kernels tetra_demod_compat runs for this plan and batch shape (TETRA_FORM_* bits).
// The default (flags 0 or TETRA_COMPAT_SEQUENTIAL) is scipy's sequential operation order in both
// recursions -- bit-identical to the reference; TETRA_COMPAT_TILED runs the decimator time-tiled
// with verified tile boundaries (compat_tiled.hip: still bit-identical); the time-blocked forms only
// under TETRA_COMPAT_BLOCKED (the blocked decimator drifts up to 1.45e-5 from scipy's fp32
// state and can flip decisions whose margin is ~1e-6 rad, so it must be asked for).
unsigned compat_forms(const tetra_compat_plan *P, size_t C, size_t N) {
    unsigned f = 0;
    const long M = P->q > 1 ? ceil_div((long)N, P->q) : (long)N;
    if (P->flags & TETRA_COMPAT_BLOCKED) {
        if (P->q > 1 && blocked_fits((int)std::min<size_t>(C, 1 << 30), (long)N, P->q)) f |= TETRA_FORM_DEC_BLOCKED;
        if (P->filt && lf_blocked_fits((int)std::min<size_t>(C, 1 << 30), M, P->ntaps)) f |= TETRA_FORM_LF_BLOCKED;
    } else if (P->flags & TETRA_COMPAT_TILED) {
        // exact either way, so outside its shapes the tiled decimator falls back silently (built-in
        // tile length: a context's tetra_compat_set_tiles is not visible to this host-only query)
        if (tiled_fits(P, C, N, 0)) f |= TETRA_FORM_DEC_TILED;
    }
    if (C >= 1 && C <= SB_MAXC) f |= TETRA_FORM_POW_PREPASS;
    return f;
}

// The sequential filtfilt takes its mixed input from a parallel k_mix pass (instead of the mixer
// inside its recursion) for batches of up to PREMIX_MAXC channels whose rows are all mixed, when the
// flags are host memory (no read-back).  Past that the batch's lanes hide the mixer's latency, and a
// float64 row written and read again would cost more than it saves (the bench's 8192 channels).
constexpr size_t PREMIX_MAXC = 64;
bool premix_fits(size_t C, const uint8_t *mix_on) {
    if (C > PREMIX_MAXC || !mix_on || is_device_ptr(mix_on)) return false;
    for (size_t c = 0; c < C; ++c)
        if (!mix_on[c]) return false;
    return true;
}

// The forms one tetra_demod_compat call runs, chosen in one place: compat_forms' decision with this
// context's tile length and the premix; the latency mode is refused outside its limits.
struct Forms { DecForm dec; LfForm lf; bool prepass; };   // decimator, filtfilt, |y|^2 before extract
int select_forms(tetra_ctx *ctx, const tetra_compat_plan *P, int fmt, size_t C, size_t N, long M,
                 const uint8_t *mix_on, Forms *F) {
    const unsigned forms = compat_forms(P, C, N);
    const bool latency = P->flags & TETRA_COMPAT_BLOCKED;
    if (P->q > 1) {
        if (latency && !blocked_fits((int)C, (long)N, P->q))
            return tetra_fail(ctx, TETRA_E_INVALID, "time-blocked decimator: C <= %d, q <= %d, N + 54 <= %d samples",
                              SB_MAXC, SB_MAXQ, SB_MAXT * SB_B);
        const bool tiled = !latency && (P->flags & TETRA_COMPAT_TILED) && fmt == TETRA_CF32 &&
                           tiled_fits(P, C, N, ctx->tl_tile);
        if (P->flags & TETRA_COMPAT_TILED) ctx->tl_ran = false;   // tetra_compat_tile_stats: this call's
        F->dec = tiled ? DEC_TILED : (forms & TETRA_FORM_DEC_BLOCKED) ? DEC_BLOCKED : DEC_SEQUENTIAL;
    }
    if (P->filt) {
        if (latency && !lf_blocked_fits((int)C, M, P->ntaps))
            return tetra_fail(ctx, TETRA_E_INVALID, "time-blocked filtfilt: C <= %d, M + 30 <= %d samples", SB_MAXC,
                              SB_MAXT * LB_B);
        F->lf = (forms & TETRA_FORM_LF_BLOCKED) ? LF_BLOCKED : premix_fits(C, mix_on) ? LF_PREMIX : LF_SEQUENTIAL;
    }
    F->prepass = forms & TETRA_FORM_POW_PREPASS;
    return TETRA_OK;
}

}  // namespace

extern "C" {

int tetra_compat_forms(const tetra_compat_plan *P, size_t C, size_t N, int32_t *forms) {
    if (!P || !forms) return TETRA_E_INVALID;
    *forms = (int32_t)compat_forms(P, C, N);
    return TETRA_OK;
}

int tetra_compat_blocked_table(const tetra_compat_plan *P, int which, double *table) {
    if (!P || !table || which < 0 || which > 2) return TETRA_E_INVALID;
    if (which == 2) {   // filtfilt's lfilter
        if (P->ntaps != LB_NS + 1) return TETRA_E_INVALID;
        lfilter_table(P->b, P->a, table);
        return TETRA_OK;
    }
    double dc[24];
    for (int i = 0; i < 24; ++i) dc[i] = which ? P->sos_f64[i] : (double)P->sos_f32[i];
    blocked_table(dc, table);
    return TETRA_OK;
}

int64_t tetra_compat_symbols(const tetra_compat_plan *P, size_t N) {
    if (!P || N == 0) return 0;
    long M = P->q > 1 ? ceil_div((long)N, P->q) : (long)N;
    return M / (P->sps < 1 ? 1 : P->sps) + 1;   // upper bound over phases
}

int tetra_demod_compat(tetra_ctx *ctx, const tetra_compat_plan *P, const void *iq, int fmt, size_t C, size_t N,
                       const double *mix_c, const uint8_t *mix_on, void *soft, uint8_t *hard, int32_t *nsym,
                       size_t smax, int32_t *soft_f32) {
    // validate and stage
    if (!ctx) return TETRA_E_INVALID;
    int rc = check_plan(ctx, P);
    if (rc) return rc;
    if (C == 0 || N == 0) return tetra_fail(ctx, TETRA_E_INVALID, "empty batch (process() handles len 0 on host)");
    if ((P->sps + P->phase_step - 1) / P->phase_step > 16) return tetra_fail(ctx, TETRA_E_INVALID, "more than 16 phases");
    const bool dec = P->q > 1;
    if (dec && (int)(fmt == TETRA_CF64) != P->dec_f64) return tetra_fail(ctx, TETRA_E_INVALID, "plan/iq precision mismatch");
    const long M = dec ? ceil_div((long)N, P->q) : (long)N;
    if ((long)smax < M / P->sps + 1 && (long)smax < M) return tetra_fail(ctx, TETRA_E_INVALID, "smax too small");
    const size_t es = compat_elem_size(ctx, fmt);
    if (!es) return TETRA_E_INVALID;
    Staging st(ctx);
    const void *x = st.in(iq, C * N * 2 * es);
    const double *mc = (const double *)st.in(mix_c, C * sizeof(double));
    const uint8_t *mo = (const uint8_t *)st.in(mix_on, C);
    if (!x || !mc || !mo) return st.finish();
    // mixed precision of the unfiltered path is per channel; require it uniform (host splits)
    uint8_t any_mix = 0, all_mix = 1;
    if (!P->filt) {
        std::vector<uint8_t> h(C);
        HIP_TRY(ctx, hipMemcpyAsync(h.data(), mo, C, hipMemcpyDefault, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (auto v : h) { any_mix |= v; all_mix &= v; }
        if (any_mix && !all_mix) return tetra_fail(ctx, TETRA_E_INVALID, "unfiltered batch with mixed freq_offset flags");
    }
    const bool f32_soft = !P->filt && !any_mix && fmt == TETRA_CF32;
    const size_t ses = f32_soft ? 4 : 8;
    void *so = st.out(soft, C * smax * 2 * ses);
    uint8_t *ho = (uint8_t *)st.out(hard, C * smax);
    int32_t *no = (int32_t *)st.out(nsym, C * 4);
    if (!so || !ho || !no) return st.finish();
    Forms F{DEC_SEQUENTIAL, LF_SEQUENTIAL, false};
    rc = select_forms(ctx, P, fmt, C, N, M, mix_on, &F);
    if (rc) return rc;
    // y: the rows the next stage reads, their layout and format
    const void *y = x;
    Lay ly = row_major(N);
    int yfmt = fmt;
    size_t yes = es;
    // stage 1: decimate (processor.py:248-257)
    if (dec) {
        void *db = ws(ctx, S_W1, grouped_elems((int)C, M) * es);
        if (!db) return TETRA_E_NOMEM;
        rc = compat_decimate(ctx, P, fmt, F.dec, x, (int)C, (long)N, db, grouped(M));
        if (rc) return rc;
        y = db;
        ly = grouped(M);
    }
    // stage 2: mixer + filtfilt (processor.py:260-264), into float64 rows
    if (P->filt || any_mix) {
        double *fb = (double *)ws(ctx, S_W3, grouped_elems((int)C, M) * 8);
        if (!fb) return TETRA_E_NOMEM;
        rc = P->filt ? compat_filtfilt(ctx, P, fmt, F.lf, y, ly, (int)C, M, mc, mo, fb, grouped(M))
                     : launch_mix(ctx, fmt, y, ly, (int)C, M, mc, mo, P->fs_dec, fb, grouped(M));
        if (rc) return rc;
        y = fb;
        ly = grouped(M);
        yfmt = TETRA_CF64;
        yes = 8;
    }
    // stage 3+4: extract_symbols + demodulate_dqpsk (processor.py:267-271)
    void *pw = F.prepass ? ws(ctx, S_W18, (size_t)C * M * yes) : nullptr;
    if (F.prepass && !pw) return TETRA_E_NOMEM;
    compat_extract_decide(ctx, P, yfmt, y, ly, (int)C, M, so, no, (long)smax, pw, ho);
    if (soft_f32) *soft_f32 = f32_soft ? 1 : 0;
    return st.finish();
}

}  // extern "C"
