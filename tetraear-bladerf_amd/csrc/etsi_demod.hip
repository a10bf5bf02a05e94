// etsi_demod.hip -- ETSI EN 300 392-2 demodulator on gfx950: channel filter and symbol timing, the
// first half of the north-star receive chain (the lower MAC that decodes its rows: etsi_lmac.hip).
//
// The reference has no such chain; this is the receiver BASELINE.json's
// north_star asks for, restating oracle/etsi_oracle.c operation for operation, so GPU and oracle
// results are bit-identical.  This unit is the host side: the plan check, the kernel choice, the tap
// image, the launches and the streaming window arithmetic.  The kernels:
//
//   k_chanfilt_r (etsi_chanfilt_r.hip)  the channel filter, one stream per wave, fused with the timing
//                stage: cf32 and SC16 chunks up to YLDS outputs.
//   k_chanfilt   (etsi_chanfilt.hip)    the same filter in workgroup-wide tiles: SC16 rows that are not
//                a multiple of four samples, and chunks longer than YLDS outputs.
//   k_timing     (etsi_timing.hip)      the timing stage alone, one wave per channel; the fused kernels
//                inline the same loop (etsi_timing.h).
#include "etsi_chanfilt.h"

// --------------------------------------------------------------------------- host side
// The canonical 2.4 MSps plan runs on the fused per-wave kernels; any other supported plan (or a
// canonical one with TETRA_ETSI_FORCE_GENERIC) on the generic-rate channel filter (etsi_rate.hip).
static bool canonical(const tetra_etsi_plan *P) {
    return P->q1 == 10 && P->L1 == 48 && P->up == 3 && P->down == 10 && P->Lp == 3 * TPP &&
           !(P->flags & TETRA_ETSI_FORCE_GENERIC);
}
static int etsi_check(tetra_ctx *ctx, const tetra_etsi_plan *P) {
    if (!P) return tetra_fail(ctx, TETRA_E_INVALID, "plan is NULL");
    if (canonical(P)) return TETRA_OK;
    if (const char *why = etsi_generic_unsupported(P))
        return tetra_fail(ctx, TETRA_E_INVALID, "unsupported ETSI plan: %s", why);
    return TETRA_OK;
}

// Which channel-filter kernel a launch takes (launch_chanfilt, tetra_etsi_kernel_info).
struct CfKernel {
    const void *fn;
    const char *name;
    bool sc16_taps;   // the stage-1 taps with SC16's sample scale folded in (the tap image's second copy)
};
// the per-wave filter (k_chanfilt_r): y in LDS (M2 <= YLDS); SC16 loads 16-B groups of 4 samples, so
// its window (N) and its rows (the pitch ld) are whole groups
static bool per_wave(int fmt, int64_t M2, size_t N, size_t ld) {
    return M2 <= YLDS && (fmt == TETRA_CF32 || (N % 4 == 0 && ld % 4 == 0));
}
// the fused demod's condition: y (and the tail's staging) fit the kernel's LDS
static bool fused_fits(int fmt, int64_t M2, int64_t sm, size_t N, size_t ld) {
    if (!per_wave(fmt, M2, N, ld)) return fmt == TETRA_SC16 && M2 + sm <= CF_LDS2_SC16;
    return sm <= WTAIL_SM;
}
static CfKernel chanfilt_kernel(int fmt, int64_t M2, size_t N, size_t ld, bool fused) {
    if (per_wave(fmt, M2, N, ld)) return {chanfilt_r_fn(fmt, fused), "k_chanfilt_r", fmt == TETRA_SC16};
    return {chanfilt_fn(fmt, fused), "k_chanfilt", false};
}

// Stage-1 taps and the per-branch stage-2 tap table (k_chanfilt), then the launch.  ld: the row pitch
// in samples (streaming windows inside a resident capture: > N).
static int launch_chanfilt(tetra_ctx *ctx, const tetra_etsi_plan *P, const void *x, int fmt, size_t C, size_t N,
                           int64_t M1, int64_t M2, float2 *y, const TimingOut *fused, size_t ld) {
    if (!canonical(P)) return fused ? TETRA_E_INVALID : launch_chanfilt_generic(ctx, P, x, fmt, C, N, M1, M2, y, ld);
    static_assert(sizeof(ctx->coef_etsi) == CF_COEF * sizeof(float), "tap image size");
    float *coef = (float *)ws(ctx, S_W12, CF_COEF * 4);   // slot of its own: the image persists
    if (!coef) return TETRA_E_NOMEM;
    float hc[CF_COEF];
    static const int i0[3] = {320, 318, 319}, off[3] = {0, 4, 7};
    for (int j = 0; j < 64; ++j) {
        hc[j] = j < 48 ? P->h1[j] : 0.f;
        hc[64 + j] = hc[j] * (1.0f / 32768.0f);   // k_chanfilt_r's SC16 taps: the sample scale folded in (exact)
    }
    // A fragment of k-step ks for lane l: A[i = l & 15][s = 4 ks + (l >> 4)], row i = 3q + c
    for (int ks = 0; ks < S2K; ++ks)
        for (int l = 0; l < 64; ++l) {
            const int i = l & 15, sidx = 4 * ks + (l >> 4), q = i / 3, c = i % 3;
            const int j = sidx - 10 * q - off[c];
            hc[128 + 64 * ks + l] = i < 15 && j >= 0 && j < TPP ? P->hp[i0[c] - 3 * j] : 0.f;
        }
    // upload only when the taps or the workspace changed: a per-call pageable copy would sit on the
    // stream in front of every launch
    if (ctx->coef_etsi_dev != coef || memcmp(hc, ctx->coef_etsi, sizeof(hc)) != 0) {
        memcpy(ctx->coef_etsi, hc, sizeof(hc));
        HIP_TRY(ctx, hipMemcpyAsync(coef, ctx->coef_etsi, CF_COEF * 4, hipMemcpyHostToDevice, ctx->stream));
        ctx->coef_etsi_dev = coef;
    }
    const CfKernel k = chanfilt_kernel(fmt, M2, N, ld, fused != nullptr);
    PROF(ctx, fused ? "etsi_demod" : "etsi_chanfilt");
    // one argument list for all seven kernels: they differ in the input pointer's type and, for the
    // per-wave SC16 kernel, in the stage-1 taps (coef + 64: the sample scale folded in)
    TimingOut to = fused ? *fused : TimingOut{};
    long n = (long)N, pitch = (long)ld;
    int m1 = (int)M1, m2 = (int)M2;
    const float *h1 = k.sc16_taps ? coef + 64 : coef, *afrag = coef + 128;
    void *args[] = {&x, &n, &m1, &m2, &h1, &afrag, &y, &to, &pitch};
    (void)hipLaunchKernel(k.fn, dim3((unsigned)C), dim3(256), args, 0, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return TETRA_OK;
}

// The demod behind tetra_demod_etsi_fmt (stream = false: C chunks of N samples, ld = N, no track,
// yoff = 0, ostride = smax) and tetra_demod_etsi_stream (one window of N samples per row of pitch ld).
static int demod_etsi(tetra_ctx *ctx, const tetra_etsi_plan *P, const void *iq, int fmt, size_t C, size_t ld, size_t N,
                      int yoff, tetra_etsi_track *track, void *soft, int8_t *softbits, uint8_t *hard, int32_t *nsym,
                      size_t smax, size_t ostride, float *diag, bool stream) {
    if (!ctx) return TETRA_E_INVALID;
    int rc = etsi_check(ctx, P);
    if (rc) return rc;
    int64_t M1, M2, sm;
    tetra_etsi_lengths(P, N, &M1, &M2, &sm);
    if (stream) {
        if (!track || C == 0 || N % 2 || ld < N || yoff < 0 || ostride < smax)
            return tetra_fail(ctx, TETRA_E_INVALID,
                              "demod_etsi_stream: track, W even <= ld, yoff >= 0, ostride >= smax");
    } else if (M2 <= 0 || N % 2 || C == 0) {
        return tetra_fail(ctx, TETRA_E_INVALID, "bad chunk for the ETSI demod");
    }
    if (fmt != TETRA_CF32 && fmt != TETRA_SC16) return tetra_fail(ctx, TETRA_E_INVALID, "iq_fmt must be cf32 or sc16");
    if (stream && fmt == TETRA_SC16 && ld % 2) return tetra_fail(ctx, TETRA_E_INVALID, "SC16 rows: ld even");
    const int64_t rows = stream ? sm + 1 : sm;   // symbols per output row (a stream's carried symbol first)
    if ((int64_t)smax < rows) return tetra_fail(ctx, TETRA_E_INVALID, "smax < %ld", (long)rows);
    Staging st(ctx);
    tetra_etsi_track *tr = stream ? (tetra_etsi_track *)st.inout(track, C * sizeof(tetra_etsi_track)) : nullptr;
    if (M2 <= 0) {   // a stream's window too short for the channel filter: no outputs; the loop's position moves on
        int32_t *no = (int32_t *)st.out(nsym, C * 4);
        if (!tr || !no) return st.finish();
        HIP_TRY(ctx, hipMemsetAsync(no, 0, C * 4, ctx->stream));
        launch_track_skip(ctx, tr, C, yoff, (int)M2);
        return st.finish();
    }
    const void *x = st.in(iq, ((C - 1) * ld + N) * (fmt == TETRA_SC16 ? 4 : 8));
    const DemodOut o = stage_demod_out(st, soft, softbits, hard, nsym, diag, C, ostride);
    if ((stream && !tr) || !x || !o.ok()) return st.finish();
    // fused: timing runs in the channel filter's workgroup on y in LDS (k_chanfilt_r: y never leaves
    // LDS; k_chanfilt<uint2>: y round-trips through a C x M2 scratch and is re-staged into the freed
    // image) (measured: cf32 with y through L2 at four workgroups per CU is 2.5 % slower)
    if (canonical(P) && fused_fits(fmt, M2, rows, N, ld)) {
        float2 *ys = nullptr;   // k_chanfilt<uint2>: y's round trip
        if (fmt == TETRA_SC16 && !per_wave(fmt, M2, N, ld) && !(ys = (float2 *)ws(ctx, S_W3, C * (size_t)M2 * 8)))
            return st.finish();
        const TimingOut to{P->gain, P->soft_scale, o.sym, o.softbits, o.hard, o.nsym, o.diag, (int)smax,
                           timing_probe(), (int)ostride, yoff, tr};
        rc = launch_chanfilt(ctx, P, x, fmt, C, N, M1, M2, ys, &to, ld);
        if (rc) return rc;
        return st.finish();
    }
    float2 *yb = (float2 *)ws(ctx, S_W3, C * (size_t)M2 * 8);
    float2 *dscr = (float2 *)ws(ctx, S_W4, C * smax * 8);
    if (!yb || !dscr) return st.finish();
    rc = launch_chanfilt(ctx, P, x, fmt, C, N, M1, M2, yb, nullptr, ld);
    if (rc) return rc;
    launch_timing(ctx, P, yb, C, (size_t)M2, o, dscr, smax, TimingOpt{tr, yoff, (int)ostride});
    return st.finish();
}

extern "C" {

int tetra_etsi_lengths(const tetra_etsi_plan *P, size_t N, int64_t *M1, int64_t *M2, int64_t *smax) {
    if (!P || !M1 || !M2 || !smax) return TETRA_E_INVALID;
    long m1 = N >= (size_t)P->L1 ? ((long)N - P->L1) / P->q1 + 1 : 0;
    long m2 = (P->up * m1 - 1 - (P->Lp - 1)) >= 0 ? (P->up * m1 - 1 - (P->Lp - 1)) / P->down + 1 : 0;
    *M1 = m1;
    *M2 = m2;
    *smax = m2 / 4 + 2;
    return TETRA_OK;
}

int tetra_etsi_kernel_info(tetra_ctx *ctx, const tetra_etsi_plan *P, int fmt, size_t N, int fused, char *name,
                           size_t name_len, int64_t *lds_bytes) {
    if (!ctx || !P || (fmt != TETRA_CF32 && fmt != TETRA_SC16)) return TETRA_E_INVALID;
    int64_t M1, M2, sm;
    tetra_etsi_lengths(P, N, &M1, &M2, &sm);
    hipFuncAttributes a;
    if (etsi_check(ctx, P)) return TETRA_E_INVALID;
    if (!canonical(P)) {
        HIP_TRY(ctx, hipFuncGetAttributes(&a, chanfilt_generic_fn(fmt)));
        if (name && name_len) snprintf(name, name_len, "%s", "k_chanfilt_g");
        if (lds_bytes) *lds_bytes = (int64_t)a.sharedSizeBytes;
        return TETRA_OK;
    }
    if (fused) fused = fused_fits(fmt, M2, sm, N, N);   // the fused form's own condition (tetra_demod_etsi_fmt)
    const CfKernel k = chanfilt_kernel(fmt, M2, N, N, fused != 0);
    HIP_TRY(ctx, hipFuncGetAttributes(&a, k.fn));
    if (name && name_len) snprintf(name, name_len, "%s", k.name);
    if (lds_bytes) *lds_bytes = (int64_t)a.sharedSizeBytes;
    return TETRA_OK;
}

int tetra_etsi_chanfilt(tetra_ctx *ctx, const tetra_etsi_plan *P, const void *iq, size_t C, size_t N, void *y) {
    return tetra_etsi_chanfilt_fmt(ctx, P, iq, TETRA_CF32, C, N, y);
}

int tetra_etsi_chanfilt_fmt(tetra_ctx *ctx, const tetra_etsi_plan *P, const void *iq, int fmt, size_t C, size_t N,
                            void *y) {
    if (!ctx) return TETRA_E_INVALID;
    int rc = etsi_check(ctx, P);
    if (rc) return rc;
    if (N % 2 || C == 0) return tetra_fail(ctx, TETRA_E_INVALID, "N must be even");
    if (fmt != TETRA_CF32 && fmt != TETRA_SC16) return tetra_fail(ctx, TETRA_E_INVALID, "iq_fmt must be cf32 or sc16");
    int64_t M1, M2, smax;
    tetra_etsi_lengths(P, N, &M1, &M2, &smax);
    if (M2 <= 0) return tetra_fail(ctx, TETRA_E_INVALID, "chunk too short for the channel filter");
    Staging st(ctx);
    const void *x = st.in(iq, C * N * (fmt == TETRA_SC16 ? 4 : 8));
    void *yo = st.out(y, C * (size_t)M2 * 8);
    if (!x || !yo) return st.finish();
    rc = launch_chanfilt(ctx, P, x, fmt, C, N, M1, M2, (float2 *)yo, nullptr, N);
    if (rc) return rc;
    return st.finish();
}

int tetra_demod_etsi(tetra_ctx *ctx, const tetra_etsi_plan *P, const void *iq, size_t C, size_t N, void *soft,
                     int8_t *softbits, uint8_t *hard, int32_t *nsym, size_t smax, float *diag) {
    return tetra_demod_etsi_fmt(ctx, P, iq, TETRA_CF32, C, N, soft, softbits, hard, nsym, smax, diag);
}

int tetra_demod_etsi_fmt(tetra_ctx *ctx, const tetra_etsi_plan *P, const void *iq, int fmt, size_t C, size_t N,
                         void *soft, int8_t *softbits, uint8_t *hard, int32_t *nsym, size_t smax, float *diag) {
    return demod_etsi(ctx, P, iq, fmt, C, N, N, 0, nullptr, soft, softbits, hard, nsym, smax, smax, diag, false);
}

int tetra_etsi_stream_window(const tetra_etsi_plan *P, int64_t x_total, int64_t y_done, int64_t n, int64_t *s,
                             int64_t *W, int64_t *yoff, int64_t *y_done_next) {
    if (!P || !s || !W || !yoff || !y_done_next || x_total < 0 || y_done < 0 || n < 0 || P->q1 < 1 || P->up < 1 ||
        P->down < 1)
        return TETRA_E_INVALID;
    // pb = q1 down input samples carry `up` outputs: a window starting at a multiple of pb has the
    // polyphase phases of a run over the whole capture, its output m is global output m + up s / pb.
    // Windows start at multiples of per = pb, doubled when odd (whole sample pairs: the kernels load
    // two samples at a time), which carry ups outputs.
    const int64_t pb = (int64_t)P->q1 * P->down, per = pb % 2 ? 2 * pb : pb, ups = P->up * (per / pb);
    int64_t st = 0;
    if (y_done > 0) {
        const int64_t a = y_done - TETRA_ETSI_MARGIN;
        st = per * (a >= 0 ? a / ups : -((-a + ups - 1) / ups));   // floor division
        if (st < 0) st = 0;
    }
    int64_t m1, m2, sm;
    tetra_etsi_lengths(P, (size_t)(x_total + n), &m1, &m2, &sm);
    *s = st;
    *W = x_total + n - st;
    *yoff = y_done - P->up * (st / pb);
    *y_done_next = m2 > y_done ? m2 : y_done;
    return TETRA_OK;
}

int tetra_demod_etsi_stream(tetra_ctx *ctx, const tetra_etsi_plan *P, const void *iq, int fmt, size_t C, size_t ld,
                            size_t W, int yoff, tetra_etsi_track *track, void *soft, int8_t *softbits, uint8_t *hard,
                            int32_t *nsym, size_t smax, size_t ostride, float *diag) {
    return demod_etsi(ctx, P, iq, fmt, C, ld, W, yoff, track, soft, softbits, hard, nsym, smax, ostride, diag, true);
}

}  // extern "C"
