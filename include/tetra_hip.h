/*
 * tetra_hip.h -- C ABI of libtetra_hip.so, the MI355X (gfx950) TETRA receive hot path.
 *
 * Drop-in boundary for the reference's demod + lower-MAC path (WizzardDr/TetraEar-BladeRF):
 *   tetraear/signal/processor.py  SignalProcessor            (processor.py:18-273)
 *   tetraear/core/decoder.py      TetraDecoder lower MAC      (decoder.py:140-295, 835-888)
 *   tetraear/core/protocol.py     parse_burst / CRC           (protocol.py:192-347)
 * plus the ETSI EN 300 392-2 receive chain the reference lacks (BASELINE.json north_star):
 *   polyphase FIR channel filter/resampler, RRC matched filter, Gardner timing recovery,
 *   differential decision with soft bits, descrambler, block deinterleaver, RCPC depuncture,
 *   K=5 rate-1/4 Viterbi, CRC-16.
 *
 * Conventions
 *   - Every entry point returns 0 on success or a negative TETRA_E* code; nothing aborts.
 *     tetra_last_error() returns the message of the last failure on that context.
 *   - Array arguments may be HOST or DEVICE pointers (the library asks HIP which); host arrays
 *     are staged through context-owned device buffers (those of up to 128 KB through a pinned
 *     host arena of the context, as async copies).  Calls with device arguments enqueue on the
 *     context's stream and return without waiting; calls that touch host memory return after
 *     their results are in host memory.
 *   - Complex arrays are interleaved (re, im).  "cf32" = complex64, "cf64" = complex128.
 *   - One context per host thread; a context is not thread-safe.  No allocation happens on a
 *     repeat call with sizes no larger than a previous call (workspaces are cached).
 */
#ifndef TETRA_HIP_H
#define TETRA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TETRA_ABI_VERSION 2

enum {
    TETRA_OK = 0,
    TETRA_E_INVALID = -1,   /* bad argument */
    TETRA_E_HIP = -2,       /* HIP runtime error */
    TETRA_E_NODEVICE = -3,  /* no usable gfx950 device */
    TETRA_E_NOMEM = -4
};

/* Sample formats of input arrays.  TETRA_SC16: interleaved int16 (I, Q), the BladeRF wire format,
 * scaled by 1/32768 as capture.py:241-269 does (exact in fp32).  Taken by the ETSI channel filter
 * (the _fmt and stream entry points), the wideband channeliser (tetra_channelize_fmt), the waterfall
 * and the AFC gate; each entry point's comment names the formats it takes. */
enum { TETRA_CF32 = 0, TETRA_CF64 = 1, TETRA_SC16 = 2 };
/* Real samples (float32 / float64), taken only by tetra_demod_dqpsk: the reference's
 * demodulate_dqpsk on a real array (processor.py:124-140 with real scalars). */
enum { TETRA_F32 = 3, TETRA_F64 = 4 };

typedef struct tetra_ctx tetra_ctx;

int tetra_abi_version(void);
/* Create a context on HIP device `device`; NULL on failure (see tetra_last_error(NULL)). */
tetra_ctx *tetra_create(int device);
void tetra_destroy(tetra_ctx *ctx);
const char *tetra_last_error(const tetra_ctx *ctx);
/* The context's hipStream_t; tetra_set_stream() makes the context enqueue on a caller stream. */
void *tetra_get_stream(tetra_ctx *ctx);
int tetra_set_stream(tetra_ctx *ctx, void *hip_stream);
int tetra_synchronize(tetra_ctx *ctx);
/* Device name / arch of the context's device (e.g. "gfx950"). */
int tetra_device_arch(tetra_ctx *ctx, char *buf, size_t n);

/* Per-stage device timing: when enabled, every kernel stage is bracketed by HIP events on the
 * context stream.  tetra_profile_read() synchronizes, then returns the accumulated milliseconds
 * and launch counts per stage since the previous read (names NUL-separated, in first-seen order). */
int tetra_profile(tetra_ctx *ctx, int enable);
/* Diagnostic: the channel filter's HBM read pattern without its arithmetic (rows workgroups, one
 * row of row_bytes each, 16-B loads; lds_bytes of LDS per workgroup caps the residency like the
 * real kernel's).  Device pointer x; timed under the "read_floor" profile stage. */
int tetra_read_floor(tetra_ctx *ctx, const void *x, size_t rows, size_t row_bytes, size_t lds_bytes);
int tetra_profile_read(tetra_ctx *ctx, char *names, size_t names_len, double *ms, int64_t *count,
                       int max_stages, int *n_stages);
/* Diagnostic: launch the one-wave marker kernel k_region_mark(tag) on the context stream.  bench.py
 * brackets its timed steps with tag 1 / tag 2, so rocprofv3 traces and counter passes of the bench
 * command can select the timed launches by dispatch order (tools/pmc_summary.py). */
int tetra_mark(tetra_ctx *ctx, int tag);

/* =====================================================================================
 * Compat demod -- bit-compatible with SignalProcessor (processor.py:221-273) in its default
 * (sequential) form and in the opt-in time-tiled form (TETRA_COMPAT_TILED); the opt-in latency mode
 * (TETRA_COMPAT_BLOCKED) is within fp32 noise only
 * ===================================================================================== */

/* Filter design and control decisions are made by the host (the same scipy.signal design calls
 * the reference makes: cheby1/sosfilt_zi for decimate, butter/lfilter_zi for filter_signal);
 * the plan carries them to the device.  Field-by-field:                                     */
typedef struct tetra_compat_plan {
    int32_t q;            /* decimation factor (processor.py:249); <= 1: decimation stage skipped */
    int32_t dec_f64;      /* 0: decimate in complex64 arithmetic (cf32 input), 1: complex128 */
    int32_t filt;         /* 1: filtfilt runs (len > padlen 15); 0: filter_signal returned input */
    int32_t ntaps;        /* butter(4) -> 5 */
    int32_t sps;          /* int(rate/18000) (processor.py:183) */
    int32_t phase_step;   /* max(1, sps//8) (processor.py:194) */
    int32_t flags;        /* TETRA_COMPAT_*: 0 = scipy's sequential order (bit-exact), TILED = the same results
                           * from time tiles with verified boundaries, BLOCKED = latency mode (not bit-exact) */
    int32_t reserved;
    double fs_dec;        /* sample rate after decimation: time base of frequency_shift */
    float sos_f32[24];    /* cheby1(8, 0.05, 0.8/q) SOS [4][6] as complex64 real parts */
    float zi_f32[8];      /* sosfilt_zi in complex64 */
    double sos_f64[24];
    double zi_f64[8];
    double b[8], a[8];    /* butter(4, cutoff) */
    double lzi[8];        /* lfilter_zi(b, a) */
    double thr[4];        /* -5*pi/8, -3*pi/8, 3*pi/8, 5*pi/8 as Python evaluates them */
} tetra_compat_plan;

/* tetra_compat_plan.flags.  The decimator and filtfilt of tetra_demod_compat run sequentially in
 * time by default (0, or TETRA_COMPAT_SEQUENTIAL): scipy's exact operation order, bit-identical to
 * the reference.  TETRA_COMPAT_BLOCKED opts into the latency mode: tiles of 256 (decimator) / 128
 * (filtfilt) samples recursed in parallel, their start states composed in float64, for C <= 64
 * channels, q <= 16 and N + 54 <= 262144 samples (TETRA_E_INVALID outside those limits); ~40x lower
 * latency for one channel but NOT bit-exact: the decimator ends up to ~1.5e-5 from scipy's fp32
 * state near the chunk start, so a decision whose phase margin is ~1e-6 rad can flip (measured: 3 in
 * 1.6 M symbols).  The component entry point tetra_decimate is always sequential.
 * TETRA_COMPAT_TILED opts into the exact time-tiled decimator: every tile of the fp32 sosfiltfilt is
 * run at once from an all-zero state `warm` samples early, the state it reaches at its first sample
 * is compared bit for bit with the state the previous tile ended in, and a tile that differs is run
 * again from that state -- so the result is the sequential one by construction, and only the speed
 * depends on the input (noisy captures: no reruns at the built-in lengths; noiseless input such as a
 * constant row: every tile rerun, as slow as the sequential form).  It applies to complex64 input,
 * 1 <= C <= 64, q in 7..10 and N longer than one tile; anywhere else, and together with
 * TETRA_COMPAT_BLOCKED, the flag is ignored (the sequential kernels give the same result).  The
 * filtfilt stage stays sequential. */
#define TETRA_COMPAT_SEQUENTIAL 1   /* the scipy-exact sequential passes (the default) */
#define TETRA_COMPAT_BLOCKED    2   /* the time-blocked latency mode (opt-in, not bit-exact) */
#define TETRA_COMPAT_TILED      4   /* tetra_compat_plan.flags: the exact time-tiled decimator (opt-in) */

/* Host-only (no device needed): the kernels tetra_demod_compat would run for `plan` on a [C][N]
 * batch, as TETRA_FORM_* bits in *forms. */
#define TETRA_FORM_DEC_BLOCKED  1   /* decimate: time-blocked (else scipy's sequential order) */
#define TETRA_FORM_LF_BLOCKED   2   /* filtfilt: time-blocked (else scipy's sequential order) */
#define TETRA_FORM_POW_PREPASS  4   /* extract_symbols: |y|^2 first in parallel (exact either way) */
#define TETRA_FORM_DEC_TILED    8   /* tetra_compat_forms: decimate runs time-tiled (bit-identical to sequential) */
int tetra_compat_forms(const tetra_compat_plan *plan, size_t C, size_t N, int32_t *forms);
/* tile / warm-up lengths of the tiled decimator on this context; 0, 0 = the built-in defaults.
 * Multiples of 64, tile >= 64, warm >= 64 (TETRA_E_INVALID otherwise).  tetra_compat_forms is
 * host-only and answers for the built-in tile length. */
int tetra_compat_set_tiles(tetra_ctx *ctx, int tile, int warm);
/* the last tiled decimate on this context, summed over streams: stats[0..3] = forward tiles checked,
 * forward tiles rerun, backward tiles checked, backward tiles rerun (all 0 if it ran sequential kernels).
 * A stream is one real component of one channel; every tile but a stream's first is checked. */
int tetra_compat_tile_stats(tetra_ctx *ctx, int32_t *stats);

/* Fused process() over a batch of C equal-length chunks.
 *   iq        [C][N] complex, format iq_fmt (TETRA_CF32 for SC16-derived capture data)
 *   mix_c     [C] imaginary part of (-1j*2*pi*freq_offset) per channel (processor.py:98-99)
 *   mix_on    [C] 1 where freq_offset != 0 (processor.py:260)
 *   soft      [C][smax] complex128: the `.symbols` attribute (processor.py:268)
 *   hard      [C][smax] uint8: process() return value; hard count = max(0, nsym-1)
 *   nsym      [C] number of soft symbols per channel
 *   soft_f32  set to 1 when `.symbols` is complex64 in the reference (no filter, no mixer)
 * smax must be >= the symbol count the plan implies (tetra_compat_symbols()). */
int tetra_demod_compat(tetra_ctx *ctx, const tetra_compat_plan *plan, const void *iq, int iq_fmt,
                       size_t C, size_t N, const double *mix_c, const uint8_t *mix_on,
                       void *soft, uint8_t *hard, int32_t *nsym, size_t smax, int32_t *soft_f32);
/* Number of soft symbols process() yields for N input samples under `plan`. */
int64_t tetra_compat_symbols(const tetra_compat_plan *plan, size_t N);
/* Host-only: the latency mode's state-transition tables.  which = 0 / 1: the time-blocked
 * decimator's Phi^(2^r), r = 0..9, row-major 8 x 8 float64 each (Phi = A^256, A the 4-section
 * cascade's one-sample zero-input transition) from the plan's complex64 / complex128 SOS, 640
 * doubles; which = 2: the time-blocked filtfilt's Psi^(2^r) (Psi = B^128, B lfilter's one-sample
 * transition of its 4 states), 160 doubles. */
int tetra_compat_blocked_table(const tetra_compat_plan *plan, int which, double *table);

/* Component entry points, one per SignalProcessor method (each over C rows of length N). */
/* scipy.signal.decimate(x, q) as called at processor.py:254: out [C][ceil(N/q)] in iq_fmt. */
int tetra_decimate(tetra_ctx *ctx, const tetra_compat_plan *plan, const void *iq, int iq_fmt,
                   size_t C, size_t N, void *out);
/* scipy.signal.decimate as tetra_decimate, on the tiled kernels where they apply. */
int tetra_decimate_tiled(tetra_ctx *ctx, const tetra_compat_plan *plan, const void *iq, int iq_fmt,
                         size_t C, size_t N, void *out);
/* frequency_shift (processor.py:85-100): out [C][N] complex128. */
int tetra_frequency_shift(tetra_ctx *ctx, const void *iq, int iq_fmt, size_t C, size_t N,
                          const double *mix_c, double fs, void *out);
/* filter_signal's filtfilt (processor.py:78-79): out [C][N] complex128; needs N > 3*ntaps. */
int tetra_filtfilt(tetra_ctx *ctx, const tetra_compat_plan *plan, const void *iq, int iq_fmt,
                   size_t C, size_t N, void *out);
/* extract_symbols (processor.py:168-219): sym [C][smax] in iq_fmt, nsym [C], best phase [C]. */
int tetra_extract_symbols(tetra_ctx *ctx, const void *x, int fmt, size_t C, size_t N, int sps,
                          int phase_step, void *sym, int32_t *nsym, int32_t *best_phase, size_t smax);
/* demodulate_dqpsk (processor.py:102-166): hard [C][S-1] for C rows of S symbols in TETRA_CF32 /
 * TETRA_CF64, or real rows in TETRA_F32 / TETRA_F64. */
int tetra_demod_dqpsk(tetra_ctx *ctx, const void *sym, int fmt, size_t C, size_t S,
                      const double *thr4, uint8_t *hard);

/* =====================================================================================
 * Compat lower MAC -- TetraDecoder.decode / find_sync / parse_burst (decoder.py, protocol.py)
 * ===================================================================================== */

#define TETRA_MAX_SYNC 16
/* Per-sync record written by tetra_lmac_compat (int32 fields). */
enum {
    TETRA_F_POS = 0,      /* sync position (bit index of the training sequence) */
    TETRA_F_START,        /* pos - 216 (decoder.py:865) */
    TETRA_F_VALID,        /* 1 if the frame is sliced (start >= 0 and start//2+255 <= S) */
    TETRA_F_NBITS,        /* len(bits[start:start+510]) (decoder_frame needs 510) */
    TETRA_F_NUMBER,       /* start // 510 (decoder.py:881) */
    TETRA_F_BTYPE,        /* BurstType value: 2 NormalDownlink, 5 Synchronization */
    TETRA_F_CRC,          /* parse_burst crc_ok */
    TETRA_F_HDR,          /* (pdu_type << 2) | encryption_mode (decoder.py:906-909) */
    TETRA_F_FIELDS = 8
};

/* Batched decode() lower MAC for C symbol streams.
 *   sym       [C][stride] int64 symbols (0..3, or 0..7 for the 8-PSK branch)
 *   nsym      [C] stream lengths
 *   k_of_max  [23] sync count threshold as a function of the stream's best correlation count,
 *             -1 for "no sync" (the 0.90/0.85/0.80/adaptive cascade, decoder.py:845-857,
 *             tabulated by the host)
 *   nsync     [C]; rec [C][TETRA_MAX_SYNC][TETRA_F_FIELDS]
 *   frame_bits[C][TETRA_MAX_SYNC][510] = bits[start:start+510]  (decode_frame 'bits')
 *   burst_bits[C][TETRA_MAX_SYNC][510] = bits of mapped[start//2:+255] (parse_burst input)  */
int tetra_lmac_compat(tetra_ctx *ctx, const int64_t *sym, const int32_t *nsym, size_t C, size_t stride,
                      const int8_t *k_of_max, int32_t *nsync, int32_t *rec, uint8_t *frame_bits,
                      uint8_t *burst_bits);
/* symbols_to_bits (decoder.py:140-169): bits [2S] int64, mapped [S] int64. */
int tetra_symbols_to_bits(tetra_ctx *ctx, const int64_t *sym, size_t S, int64_t *bits, int64_t *mapped);
/* find_sync main scan (decoder.py:226-259) at integer count threshold kthr:
 * pos [maxpos], *npos hits, *maxc = max evaluated correlation count. */
int tetra_find_sync(tetra_ctx *ctx, const uint8_t *bits, size_t nbits, int kthr, int64_t *pos,
                    int maxpos, int32_t *npos, int32_t *maxc);
/* Pattern match counts (the np.sum(window == pattern) of decoder.py:239 / protocol.py:262):
 * counts[f] = #{j < 22 : bits[f][offset+j] == pattern22[j]} over F rows of L bytes. */
int tetra_match_count(tetra_ctx *ctx, const uint8_t *bits, size_t F, size_t L, const uint8_t *pattern22,
                      size_t offset, int32_t *counts);
/* parse_burst over F bursts of 255 symbols (protocol.py:192-244): btype [F], crc_ok [F],
 * bits [F][510] burst bits (training sequence/data are slices of these). */
int tetra_parse_bursts(tetra_ctx *ctx, const int64_t *sym, size_t F, int32_t *btype, uint8_t *crc_ok,
                       uint8_t *bits);
/* _calculate_crc16 over F rows of L bits (reversed != 0: payload reversed): crc [F]. */
int tetra_crc16(tetra_ctx *ctx, const uint8_t *bits, size_t F, size_t L, int reversed, uint16_t *crc);
/* _check_crc over F rows of L bits: ok [F]. */
int tetra_check_crc(tetra_ctx *ctx, const uint8_t *bits, size_t F, size_t L, uint8_t *ok);

/* MAC PDU header extraction of TetraProtocolParser.parse_mac_pdu (protocol.py:349-596; SURVEY.md
 * §8f rank 4) over F frames of data bits, one byte per bit (any nonzero byte reads as 1, in the
 * header fields and the data bytes alike), one row of `stride` bytes each, nbits[f] valid.
 * Stateless per frame: the fragment buffer, the MCC/MNC/colour-code state and the statistics are
 * applied in order by the host (tetraear.core.protocol.parse_mac_pdu_batch).
 *   fields [F][TETRA_MAC_FIELDS] (below); data [F][data_stride] = BitArray(data bits).tobytes()
 *   (MSB first, last byte zero-padded), data_stride >= (stride + 7) / 8. */
enum {
    TETRA_MAC_STATUS = 0,   /* 0 PDU; 1 None, no state touched (len < 8, truncated address/length,
                               length check protocol.py:433/525, short SYSINFO); 2 None after the
                               SYSINFO state write (MCC outside 200..799 or MNC > 999, :489-494) */
    TETRA_MAC_PTYPE,        /* PDUType value: 0 RESOURCE, 1 FRAG, 2 END (header 3), 3 BROADCAST (header 2) */
    TETRA_MAC_MODE,         /* (bits[2] << 1) | bits[3] (:389) */
    TETRA_MAC_FILL,         /* bits[4] (RESOURCE, FRAG, END), else 0 */
    TETRA_MAC_ADDR,         /* 24-bit address (RESOURCE), else -1 */
    TETRA_MAC_LENGTH,       /* 6-bit length indicator (RESOURCE, END), else 0 */
    TETRA_MAC_DATA_BITS,    /* number of data bits packed into data[f] */
    TETRA_MAC_SYSINFO,      /* 1 if the SYSINFO MCC/MNC/colour code below were read (:482-485) */
    TETRA_MAC_MCC,
    TETRA_MAC_MNC,
    TETRA_MAC_CC,
    TETRA_MAC_FIELDS = 12
};
int tetra_mac_headers(tetra_ctx *ctx, const uint8_t *bits, const int32_t *nbits, size_t F, size_t stride,
                      int32_t *fields, uint8_t *data, size_t data_stride);

/* Signal-present / AFC gate of the capture loop (/root/reference/tetraear/ui/modern.py:1952-2028,
 * SURVEY.md §8f rank 1), per channel on the 2048-point Hann spectrum of its first 2048 samples
 * (the k_waterfall row, fused): centre band of int(25000 / (fs / 2048)) bins around bin 1024, noise
 * floor from the bins 10 beyond it on both sides, present iff snr > 15 dB and peak > -70 dBFS and
 * peak - band mean > 3 dB, AFC offset = the peak bin's frequency when present.  stats [C][FIELDS]
 * (host or device); power [C][2048] the dB rows or NULL; mixer_coef / mixer_on [C] (or NULL) the
 * offset as tetra_demod_compat's mixer arguments (-2 pi f, f != 0), so process() runs on the gate's
 * AFC with no host round trip.  N < 2048: no detection (all zero). */
enum {
    TETRA_GATE_VALID = 0,     /* 1 when a centre band exists (N >= 2048 and >= 2 band bins) */
    TETRA_GATE_SIGNAL,        /* mean dB of the centre band */
    TETRA_GATE_PEAK,          /* max dB of the centre band */
    TETRA_GATE_PEAK_BIN,      /* its first index (0..2047, fftshifted) */
    TETRA_GATE_PEAK_FREQ,     /* its frequency fftshift(fftfreq(2048, 1/fs))[bin], Hz */
    TETRA_GATE_NOISE,         /* noise floor (mean dB outside the band +- 10 bins, -100 if none) */
    TETRA_GATE_SNR,           /* signal - noise */
    TETRA_GATE_ABOVE,         /* peak - signal */
    TETRA_GATE_PRESENT,       /* 1: signal present (the three thresholds) */
    TETRA_GATE_AFC,           /* the freq_offset process() gets: PEAK_FREQ when present, else 0 */
    TETRA_GATE_FIELDS = 10
};
int tetra_afc_gate(tetra_ctx *ctx, const void *iq, int iq_fmt, size_t C, size_t N, double fs, float *power,
                   double *stats, double *mixer_coef, uint8_t *mixer_on);

/* The scanner's TETRA signal detector over a batch of candidate channels (SURVEY.md §8f rank 2;
 * replaces the per-sample Python loops of /root/reference/tetraear/signal/scanner.py:42-147 and
 * 204-231): per channel of iq [C][N] (TETRA_CF32 / TETRA_CF64) the counts the detector's decisions
 * are made from -- the pi/4-DQPSK cluster test over consecutive samples, the best 31-bit match of
 * sync_pattern (bit j of the word = pattern bit j) over the bits of the samples strided by
 * `downsample`, and the mean powers of the chunk and of its five equal windows -- into
 * stats [C][TETRA_SCAN_FIELDS] (host or device).  At most 131072 sync bits per channel. */
enum {
    TETRA_SCAN_MOD_MATCHES = 0,   /* phase differences within pi/8 of a multiple of pi/4 in [-pi, 3pi/4] */
    TETRA_SCAN_MOD_DIFFS,         /* N - 1 */
    TETRA_SCAN_SYNC_MATCHES,      /* best match count (0..31) over the window starts */
    TETRA_SCAN_SYNC_WINDOWS,      /* window starts searched: max(0, nbits - 31) */
    TETRA_SCAN_SYNC_BITS,         /* bits: strided samples - 1 */
    TETRA_SCAN_POWER,             /* mean |x|^2 */
    TETRA_SCAN_POWER_W0,          /* mean |x|^2 of window i = [i (N/5), (i+1) (N/5)), i = 0..4 */
    TETRA_SCAN_FIELDS = TETRA_SCAN_POWER_W0 + 5
};
int tetra_scan_detect(tetra_ctx *ctx, const void *iq, int iq_fmt, size_t C, size_t N, int downsample,
                      uint32_t sync_pattern, double *stats);

/* =====================================================================================
 * ETSI EN 300 392-2 receive chain (north star; no reference counterpart)
 * ===================================================================================== */

/* Receiver design (filled by the host: tetraear.signal.etsi.etsi_plan).  Stage 1: L1-tap FIR
 * decimating by q1 (fs -> fs1 = fs / q1); stage 2: RRC (0.35) polyphase prototype of Lp taps at
 * up * fs1 = 4 * down * 18 kHz, resampled x up/down to 72 kHz (4 samples/symbol); then timing.
 *   2.4 MSps: q1 = 10, L1 = 48, 3/10, Lp = 321 -- the canonical plan, run by the fused per-wave
 *             kernels (k_chanfilt_r / k_chanfilt);
 *   any other plan with q1 <= 13, L1 <= 64, Lp <= 4096 and (Lp - 1) / up <= 256 (e.g. the
 *             reference CLI's 1.8-2.4 MSps in 0.1 MHz steps, modern.py:5518-5519, 5630-5638): the
 *             generic-rate channel filter k_chanfilt_g (y through HBM) + k_timing.
 * flags bit 0 (TETRA_ETSI_FORCE_GENERIC): run a canonical plan on the generic kernel too (tests). */
#define TETRA_ETSI_FORCE_GENERIC 1
typedef struct tetra_etsi_plan {
    int32_t q1, L1, Lp, up, down;
    float gain;           /* block-Gardner loop gain */
    float soft_scale;     /* int8 soft-bit scale: soft = rint(x * soft_scale / mean|d|) */
    int32_t flags;
    float h1[64];
    float hp[4096];
} tetra_etsi_plan;

#define TETRA_ETSI_MAXB 8    /* bursts per channel chunk */
#define TETRA_ETSI_MAXJ 16   /* coded blocks per channel chunk */
/* block kinds */
enum { TETRA_SCH_F = 0, TETRA_SCH_HD = 1, TETRA_BSCH = 2 };
/* burst kinds */
enum { TETRA_NDB_N = 0, TETRA_NDB_P = 1, TETRA_SB = 2 };

/* M1 (240 kHz samples), M2 (72 kHz samples) and the symbol capacity smax for N input samples. */
int tetra_etsi_lengths(const tetra_etsi_plan *plan, size_t N, int64_t *M1, int64_t *M2, int64_t *smax);
/* Channel filter + RRC resampler: iq [C][N] cf32 -> y [C][M2] cf32. */
int tetra_etsi_chanfilt(tetra_ctx *ctx, const tetra_etsi_plan *plan, const void *iq, size_t C, size_t N, void *y);
/* Timing recovery + differential decision: y [C][M2] ->
 *   soft [C][smax] cf32 symbol-spaced samples (the ETSI `.symbols`), softbits [C][2*smax] int8
 *   (>0: bit 0), hard [C][smax] dibit symbols 0..3 (count nsym-1), nsym [C],
 *   diag [C][4] (timing phase, final Gardner correction, CFO rotation re/im) or NULL.
 *   Entries past a channel's nsym (symbols) and nsym-1 (soft bits, dibits) are unspecified.
 *   TETRA_TIMING_PROBE=1 (diagnostic): diag holds four 32-bit wall-clock stamps per channel instead. */
int tetra_etsi_timing(tetra_ctx *ctx, const tetra_etsi_plan *plan, const void *y, size_t C, size_t M2,
                      void *soft, int8_t *softbits, uint8_t *hard, int32_t *nsym, size_t smax, float *diag);
/* tetra_etsi_timing for the wideband chain's chunks, with the Oerder-Meyr class sums formed from
 * the resampler's group partials om (tetra_channelize_om) instead of a pass over y: y [C][M2] is
 * C / nchunk carrier rows of nchunk consecutive chunks, om [C / nchunk][ngrp] float4 the rows'
 * partials over groups of U outputs (U a multiple of 4, <= 64; ngrp U >= nchunk M2; M2 a multiple
 * of 4).  The class sums follow oracle/etsi_oracle.c eo_om_grouped (a summation order of the same
 * |y|^2 class sums; same outputs as tetra_etsi_timing otherwise; no reference counterpart). */
int tetra_etsi_timing_om(tetra_ctx *ctx, const tetra_etsi_plan *plan, const void *y, size_t C, size_t M2,
                         const void *om, size_t nchunk, size_t ngrp, int U, void *soft, int8_t *softbits,
                         uint8_t *hard, int32_t *nsym, size_t smax, float *diag);
/* tetra_etsi_timing over overlapping chunks of M carrier rows y [M][rowlen]: output row k nchunk + c
 * is the timing of y[k][c stride, min(c stride + len, rowlen)) (len > stride: consecutive chunks
 * share len - stride samples, so a burst that straddles one chunk's end lies whole in it -- the
 * wideband chain's seams lose no burst).  om: NULL (each chunk's own Oerder-Meyr pass over y) or
 * the rows' resampler partials [M][ngrp] float4 as in tetra_etsi_timing_om (stride a multiple of 4,
 * ngrp U >= rowlen).  smax >= len / 4 + 2.  Outputs as tetra_etsi_timing with C = M nchunk; a
 * chunk's outputs are the oracle's timing of its samples (no reference counterpart: the reference
 * demodulates one narrowband capture at a time, tetraear/signal/processor.py:253-331). */
int tetra_etsi_timing_chunks(tetra_ctx *ctx, const tetra_etsi_plan *plan, const void *y, size_t M, size_t rowlen,
                             size_t nchunk, size_t stride, size_t len, const void *om, size_t ngrp, int U, void *soft,
                             int8_t *softbits, uint8_t *hard, int32_t *nsym, size_t smax, float *diag);
/* Fused demod (chanfilt + timing) over a batch.
 *   Amplitude range (cf32 is taken as it comes, not assumed to lie in +-1): for a nominal row
 *   (amplitude about 0.5) scaled by 2^k, every output is scale-exact -- the same dibits, soft bits,
 *   nsym and diag, the symbols times 2^k, bit for bit -- for k in [-16, +10] (amplitude 8e-6 ... 500;
 *   SC16 at a few LSB is inside).  Above it the CFO correction is off (the 4th-power sums overflow:
 *   the rotation is the identity, dibits stay right while the offset is small); from about 2^29 the
 *   soft bits read 0, from about 2^58 nsym is 0 and diag[0] NaN.  Below it the rotation decays to
 *   the identity (2^-19 ... 2^-40), then the soft bits read 0, and under about 2^-100 the row
 *   decodes as silence.  No amplitude returns wrong dibits with symbols present.  DESIGN.md §5.15.
 *   A row of fewer than 16 filter outputs has nsym 0 and diag zeros. */
int tetra_demod_etsi(tetra_ctx *ctx, const tetra_etsi_plan *plan, const void *iq, size_t C, size_t N,
                     void *soft, int8_t *softbits, uint8_t *hard, int32_t *nsym, size_t smax, float *diag);
/* The same two entry points for an explicit input format (TETRA_CF32 or TETRA_SC16); the
 * format-less forms above take cf32. */
int tetra_etsi_chanfilt_fmt(tetra_ctx *ctx, const tetra_etsi_plan *plan, const void *iq, int iq_fmt, size_t C,
                            size_t N, void *y);
int tetra_demod_etsi_fmt(tetra_ctx *ctx, const tetra_etsi_plan *plan, const void *iq, int iq_fmt, size_t C,
                         size_t N, void *soft, int8_t *softbits, uint8_t *hard, int32_t *nsym, size_t smax,
                         float *diag);
/* Differential decision on n given symbol-spaced samples x (TETRA_CF32 / TETRA_CF64): hard [n-1]
 * dibits by EN 300 392-2 Table 5.1 (the fused demod's decision, no CFO rotation).  Replaces the
 * reference's demodulate_dqpsk (/root/reference/tetraear/signal/processor.py:102-166) in ETSI mode,
 * whose shifted decision regions SURVEY.md §0.3 documents. */
int tetra_etsi_decide(tetra_ctx *ctx, const void *x, int iq_fmt, size_t n, uint8_t *hard);
/* The channel-filter kernel a demod (fused != 0) or chanfilt call on N-sample rows of iq_fmt runs:
 * its symbol name and static LDS bytes per workgroup (the occupancy the bench's read floor mimics). */
int tetra_etsi_kernel_info(tetra_ctx *ctx, const tetra_etsi_plan *plan, int iq_fmt, size_t N, int fused, char *name,
                           size_t name_len, int64_t *lds_bytes);
/* Cell configuration: scrambling code init per channel ((MCC<<20|MNC<<6|CC)<<2|3). */
int tetra_etsi_set_cells(tetra_ctx *ctx, const uint32_t *scramb_init, size_t C);
/* Lower MAC: burst sync + descramble + deinterleave + depuncture + Viterbi + CRC per channel.
 *   nburst [C], bursts [C][TETRA_ETSI_MAXB][2] (start bit, burst kind),
 *   nblock [C], blocks [C][TETRA_ETSI_MAXJ][4] (block kind, crc_ok, burst index, block index),
 *   type1 [C][TETRA_ETSI_MAXJ][268] decoded type-1 bits.
 * Entries past nburst[c] / nblock[c], and a block's type-1 bytes past its length, are not written.
 * Rows are at most 2050 symbols wide (smax); every one of a row's nsym[c] - 1 dibits is scanned.
 * Soft bits are expected in [-127, 127], which is what the demodulator writes: a -128 is its own
 * negative under descrambling (it stays negative where the scrambling bit is 1), in the library and
 * in the oracle alike. */
int tetra_lmac_etsi(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, const int32_t *nsym,
                    size_t C, size_t smax, int32_t *nburst, int32_t *bursts, int32_t *nblock,
                    int32_t *blocks, uint8_t *type1);
/* Lower MAC with cell acquisition: the same outputs as tetra_lmac_etsi, without a configured cell.
 * cell_init [C] (in/out, host or device) holds each channel's scrambling init before the chunk
 * (3 = colour code 0 / not yet acquired).  The chunk's BSCH blocks are decoded first (colour code
 * 0, as every receiver must before it knows the cell); the last CRC-good one sets the channel's
 * extended colour code from its type-1 bits -- MAC-SYNC colour code bits 4..9, D-MLE-SYNC MCC bits
 * 31..40 and MNC bits 41..54 (EN 300 392-2 §21.4.4.2, §18.4.2.1) -- and the SCH/F / SCH/HD blocks
 * are then descrambled with it (§8.2.5.2).  cell_init returns the updated inits, so a stream of
 * chunks keeps the cell it acquired, as the reference parser keeps the MCC/MNC/colour code it
 * reads from a SYSINFO broadcast (/root/reference/tetraear/core/protocol.py:479-485).  The
 * scrambling table is cached per channel in the context and regenerated on the device only for
 * channels whose init changed. */
int tetra_lmac_etsi_acquire(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, const int32_t *nsym,
                            size_t C, size_t smax, uint32_t *cell_init, int32_t *nburst, int32_t *bursts,
                            int32_t *nblock, int32_t *blocks, uint8_t *type1);
/* Cell acquisition per group of rows (a new symbol of ABI version 2; nothing existing changed shape).
 * Rows g G .. g G + G - 1 are G consecutive pieces of one carrier, in time order -- the wideband
 * chain's (carrier, chunk) rows, G = chunks per carrier -- and share one cell: cell_init [C / G]
 * (in/out) and ngood [C / G] (out), host or device.  tetra_lmac_etsi_acquire's rule taken from a row
 * to a group: the burst scan on every row, every row's BSCH blocks decoded with colour code 0, then
 * per group the rows in ascending order and each row's bursts in order -- the last CRC-good BSCH
 * sets cell_init[g] (the same type-1 fields), none keeps it (3 = unknown) -- and every SCH/F and
 * SCH/HD block of every row of the group, the rows before the synchronisation burst's included, is
 * descrambled with cell_init[g].  ngood[g] counts the CRC-good BSCH blocks of the group in this
 * call: an all-zero cell (MCC = MNC = colour code = 0) has the init of "unknown", so the count, not
 * the init, says that a cell was heard.  Outputs as tetra_lmac_etsi's, per row.  G >= 1 and
 * C % G == 0, else TETRA_E_INVALID with nothing written; G = 1 is tetra_lmac_etsi_acquire bit for
 * bit.  Replaces, for the wideband chain, handing tetra_etsi_set_cells one known init per carrier:
 * the state the reference parser keeps from a broadcast
 * (/root/reference/tetraear/core/protocol.py:479-485), kept per carrier over all of its rows. */
int tetra_lmac_etsi_acquire_groups(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, const int32_t *nsym,
                                   size_t C, size_t smax, size_t G, uint32_t *cell_init /*[C/G] in/out*/,
                                   int32_t *ngood /*[C/G] out*/, int32_t *nburst, int32_t *bursts, int32_t *nblock,
                                   int32_t *blocks, uint8_t *type1);
/* ---------------------------------------------------------------- streaming (one continuous capture)
 * The reference's callers stream a continuous capture in chunks (modern.py:1901-1919,
 * continuous_capture.py:20); these entry points decode consecutive chunks of each channel as ONE
 * symbol stream, so no burst is lost at a chunk seam (oracle/etsi.py: Stream restates them).
 *   1. tetra_etsi_stream_window: where chunk k's channel-filter window starts.  The window re-reads
 *      the previous chunk's last samples from s, a multiple of P = q1 * down input samples, so its
 *      filter phases equal a run over the whole capture; yoff = its first new 72 kHz output.
 *   2. tetra_demod_etsi_stream: the fused demod over the window (rows of `ld` samples: a capture
 *      resident as [C][ld] is windowed in place) with each channel's timing loop carried in track.
 *   3. tetra_lmac_etsi_stream: the lower MAC over rows that hold the previous chunk's unconsumed
 *      dibits in front of the new ones; the greedy burst scan resumes at the bit it stopped at. */
typedef struct tetra_etsi_track {
    float base;       /* next symbol's Gardner base position, 72 kHz samples from the end of the last chunk's outputs */
    float delta;      /* block-Gardner loop offset */
    float prev_re, prev_im;   /* the last symbol of the previous chunk (dibit 0 of the next spans the seam) */
    int32_t acquired;         /* 0: the next chunk acquires the phase (Oerder-Meyr) and starts a new chain */
    int32_t reserved[3];
} tetra_etsi_track;
#define TETRA_ETSI_RESERVE 256   /* dibits ahead of a streaming output row (the lower MAC's carried tail) */
#define TETRA_ETSI_MARGIN 8      /* 72 kHz samples a window re-computes before its first new output */

/* Host-only window arithmetic: for a stream of x_total samples already received (y_done 72 kHz
 * outputs produced) and a next chunk of n samples: *s = the window's first sample (global index),
 * *W = its length (x_total + n - s), *yoff = the window index of output y_done, *y_done_next. */
int tetra_etsi_stream_window(const tetra_etsi_plan *plan, int64_t x_total, int64_t y_done, int64_t n, int64_t *s,
                             int64_t *W, int64_t *yoff, int64_t *y_done_next);
/* Fused demod of one window per channel: iq points at the window's first sample of channel 0, rows
 * ld samples apart (ld >= W, a multiple of 4 for SC16); track [C] (in/out, host or device).  Outputs
 * as tetra_demod_etsi_fmt, rows `ostride` symbols apart with capacity smax: with track[c].acquired,
 * symbol 0 is the carried last symbol of the previous chunk, so the nsym-1 dibits start with the one
 * across the seam. */
int tetra_demod_etsi_stream(tetra_ctx *ctx, const tetra_etsi_plan *plan, const void *iq, int iq_fmt, size_t C,
                            size_t ld, size_t W, int yoff, tetra_etsi_track *track, void *soft, int8_t *softbits,
                            uint8_t *hard, int32_t *nsym, size_t smax, size_t ostride, float *diag);
/* Lower MAC over streaming rows: row c of hard (softbits) is `stride` dibits (2 stride bytes); this
 * chunk's nsym[c]-1 dibits start at TETRA_ETSI_RESERVE, the previous chunk's tail is in front of
 * them and lead[c] (in/out) is the row bit the scan starts at (2 * TETRA_ETSI_RESERVE for a new
 * stream).  After the scan the unconsumed dibits (from the first bit not examined) are copied in
 * front of TETRA_ETSI_RESERVE in next_soft / next_hard (the rows the next chunk's demod writes;
 * they may be these rows) and lead[c] set for the next chunk.  bursts[.][0] is the burst's start
 * bit relative to this chunk's first new dibit (negative: it began in the carried tail).
 * cell_init: NULL (configured cells) or the acquisition state, as tetra_lmac_etsi_acquire. */
int tetra_lmac_etsi_stream(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, const int32_t *nsym,
                           size_t C, size_t stride, int32_t *lead, int8_t *next_soft, uint8_t *next_hard,
                           uint32_t *cell_init, int32_t *nburst, int32_t *bursts, int32_t *nblock, int32_t *blocks,
                           uint8_t *type1);

/* ---------------------------------------------------------------- loss-of-lock monitor (new symbols of ABI
 * version 2; nothing existing changed shape).  A streaming channel's timing loop, filter history and
 * lower-MAC tail are carried from chunk to chunk, and nothing in tetra_demod_etsi_stream sets
 * track.acquired back to 0: after a retune, an SDR sample drop or a signal that went away, the loop is
 * joined onto stale state, and a slip of about half a symbol cannot be tracked out at all (the block-
 * Gardner offset is clamped to +-1.5 of the 4 samples a symbol has).  tetra_etsi_lock
 * judges every chunk from its soft bits and the loop's offset and hands a channel that lost lock back
 * to acquisition (k_etsi_lock, one launch; tests/_etsi_lock_model.py restates it; no reference
 * counterpart: the reference demodulates every chunk on its own,
 * /root/reference/tetraear/signal/processor.py:253-331).
 *
 * Call it after tetra_demod_etsi_stream, on that call's softbits, nsym, ostride and track, on the same
 * context (host or device pointers, as that call takes them; with device pointers it enqueues and
 * returns without waiting).
 *
 * Sums (exact integers).  N = min(max(nsym[c] - 1, 0), ostride) dibits of row c, bytes (s0, s1) each;
 * a = |s0|, b = |s1| (-128 reads 128), hi = max(a, b), lo = min(a, b).  A dibit with hi < weak counts
 * in WEAK; every other one adds lo to SMIN and hi to SMAX.  A clean pi/4-DQPSK decision has |s0| =
 * |s1|, so SMIN / SMAX ("balance") is near 1 in lock and near 0.44 on noise or at a wrong timing phase.
 * Nothing past byte 2 N of a row is read.
 *
 * Rule, per channel.  An all-zero state reads as {searching = 1}: the first chunk of a stream is an
 * acquisition chunk.  fresh = state.searching on entry; judged = N >= nmin; chunks += 1 always, and an
 * unjudged chunk changes nothing else.  A judged chunk is bad if 2 WEAK > N, or SMAX == 0, or
 * (int64) SMIN den < (int64) num SMAX, or railed: |track[c].delta| >= 1.5f, the loop's own clamp (an
 * exact compare; NaN is not railed).
 *   good:             searching = 0, bad_run = 0;
 *   bad and fresh:    track[c].acquired = 0, searching = 1 -- the channel keeps searching, every chunk
 *                     acquiring afresh as every chunk did before streaming;
 *   bad, not fresh:   bad_run += 1, and at bad_run >= patience the channel is DROPPED:
 *                     track[c].acquired = 0, searching = 1, bad_run = 0, relocks += 1.
 * rec [C][TETRA_LOCK_FIELDS] (fully written): SMIN, SMAX, N, WEAK, the TETRA_LOCK_* flag bits, bad_run
 * and relocks after the chunk, 0.
 * TETRA_E_INVALID with nothing written: a NULL softbits, nsym, track, state or rec, C == 0, ostride == 0
 * or above 2^23 (the sums are 32-bit), C above 2^24, den <= 0, num < 0, patience < 1. */
typedef struct tetra_etsi_lock_state {
    int32_t searching;   /* 1: the channel has no lock; the next judged chunk is an acquisition chunk */
    int32_t bad_run;     /* consecutive bad chunks since the last good one (locked channels) */
    int32_t relocks;     /* times the channel was dropped */
    int32_t chunks;      /* calls so far */
    int32_t reserved[4];
} tetra_etsi_lock_state;
enum {
    TETRA_LOCK_SMIN = 0, TETRA_LOCK_SMAX, TETRA_LOCK_N, TETRA_LOCK_WEAK, TETRA_LOCK_FLAGS, TETRA_LOCK_BAD_RUN,
    TETRA_LOCK_RELOCKS, TETRA_LOCK_FIELDS = 8
};
#define TETRA_LOCK_JUDGED 1      /* N >= nmin */
#define TETRA_LOCK_BAD 2
#define TETRA_LOCK_RAILED 4      /* |delta| >= 1.5 after the chunk (reported for unjudged chunks too) */
#define TETRA_LOCK_FRESH 8       /* the channel was searching on entry */
#define TETRA_LOCK_DROPPED 16    /* this chunk dropped the channel */
#define TETRA_LOCK_SEARCHING 32  /* state.searching after the chunk */
#define TETRA_ETSI_LOCK_NUM_DEFAULT 1        /* a stated choice, backed by the table of §5.28 */
#define TETRA_ETSI_LOCK_DEN_DEFAULT 2        /* a stated choice, backed by the table of §5.28 */
#define TETRA_ETSI_LOCK_WEAK_DEFAULT 8       /* a stated choice, backed by the table of §5.28 */
#define TETRA_ETSI_LOCK_NMIN_DEFAULT 64      /* a stated choice, backed by the table of §5.28 */
#define TETRA_ETSI_LOCK_PATIENCE_DEFAULT 1   /* a stated choice, backed by the table of §5.28 */
int tetra_etsi_lock(tetra_ctx *ctx, const int8_t *softbits, const int32_t *nsym, size_t C, size_t ostride /*symbols*/,
                    int32_t num, int32_t den, int32_t weak, int32_t nmin, int32_t patience,
                    tetra_etsi_track *track /*[C] in/out*/, tetra_etsi_lock_state *state /*[C] in/out*/,
                    int32_t *rec /*[C][TETRA_LOCK_FIELDS] out*/);

/* ---------------------------------------------------------------- cell vote (new symbols of ABI version 2;
 * nothing existing changed shape).  tetra_lmac_etsi_acquire and _acquire_groups let the LAST CRC-good BSCH
 * set a cell: one false CRC pass on a badly received block (2^-16 per failed block), or a neighbour
 * cell's synchronisation burst heard on the carrier, replaces the cell, and every SCH block after it is
 * descrambled wrongly until the next good BSCH.  The vote entry points are those calls with every
 * CRC-good BSCH weighed by its soft bits and the cell kept so far defending with a score.
 *
 * The rule (exact integers).  State per group g of G rows: cell_init[g] (uint32, in/out, as above; 3 =
 * unknown) and score[g] (int32, in/out; 0 = fresh; a negative value is read as 0).
 *   Ballots: the group's CRC-good BSCH blocks in order -- rows ascending, each row's bursts in order (the
 *     blocks ngood counts).  Block i has c_i, the init from its type-1 bits (the fields of
 *     tetra_lmac_etsi_acquire), and w_i = max(1, WSUM_i - 2 WERR_i), where WSUM and WERR are
 *     tetra_etsi_link_quality's block-record quantities for the block: its 60 type-1 bits re-encoded as
 *     tetra_etsi_encode_blocks does (kind 2, init 3) into 120 type-5 bits and held against the 120 soft
 *     bytes the trellis read (row bits start + 94 ..., from the streaming origin for streaming rows);
 *     WSUM = sum of |s| over the 120, WERR = sum of |s| over the non-zero s whose sign disagrees with the
 *     codeword.  w_i is the correlation of the soft bits with the codeword the decoder chose -- the
 *     Viterbi's own path metric, no tuned constant -- at most 120 * 127 = 15240 for soft bits in
 *     [-127, 127].
 *   Totals (int64): T(c) = sum of w_i over c_i == c, plus score[g] if c == cell_init[g].  Candidates: the
 *     incoming cell_init[g] and every distinct c_i.
 *   Winner: the largest T; on a tie the incoming cell if it is among the tied, else the tied candidate
 *     whose last ballot comes latest.
 *   Update: without a ballot cell_init[g] and score[g] stay as they were; else cell_init[g] = winner and
 *     score[g] = min(cap, max(1, T(winner) - sum of T(c) over c != winner)): a weighted majority vote of
 *     Boyer-Moore type -- losers wear the incumbent down -- and cap (> 0) bounds incumbency, so a real
 *     change of cell wins after a bounded amount of contrary evidence.
 *   Outputs: ngood[g] = the number of ballots, agree[g] = the ballots with c_i == winner (0 without one).
 * With score 0 and one ballot this is tetra_lmac_etsi_acquire_groups's rule.  Every SCH/F and SCH/HD
 * block of every row of the group is then descrambled with cell_init[g], exactly as there.  A burst in
 * samples that two overlapping chunks share votes in both rows, as it counts in ngood twice.
 * TETRA_ETSI_VOTE_CAP_DEFAULT: eight full-scale BSCH blocks, about two multiframes of frame-18
 * broadcasts at full strength -- a stated choice, not a measurement. */
#define TETRA_ETSI_VOTE_CAP_DEFAULT 121920
/* tetra_lmac_etsi_acquire_groups with the vote: score [C / G] in/out and agree [C / G] out beside
 * cell_init and ngood, host or device.  TETRA_E_INVALID with nothing written: a NULL cell_init, score,
 * ngood or agree, cap <= 0, G == 0, C % G != 0, G > 32 (a group's ballot list is fixed-size;
 * tetra_lmac_etsi_acquire_groups keeps serving larger groups), and whatever tetra_lmac_etsi refuses. */
int tetra_lmac_etsi_vote_groups(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, const int32_t *nsym,
                                size_t C, size_t smax, size_t G, int32_t cap, uint32_t *cell_init /*[C/G] in/out*/,
                                int32_t *score /*[C/G] in/out*/, int32_t *ngood /*[C/G] out*/,
                                int32_t *agree /*[C/G] out*/, int32_t *nburst, int32_t *bursts, int32_t *nblock,
                                int32_t *blocks, uint8_t *type1);
/* tetra_lmac_etsi_stream in acquisition mode with the vote, a group being one streaming row: cell_init
 * [C] and score [C] in/out (NULL: TETRA_E_INVALID, as cap <= 0), agree [C] out (may be NULL).  A BSCH that
 * began in the carried tail votes in the call that decodes it, with the soft bytes carried with it. */
int tetra_lmac_etsi_stream_vote(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, const int32_t *nsym,
                                size_t C, size_t stride, int32_t *lead, int8_t *next_soft, uint8_t *next_hard,
                                int32_t cap, uint32_t *cell_init, int32_t *score, int32_t *agree, int32_t *nburst,
                                int32_t *bursts, int32_t *nblock, int32_t *blocks, uint8_t *type1);

/* ---------------------------------------------------------------- TDMA timebase + MAC PDU headers
 * What a receiver reads next from the lower MAC's outputs, on the device: per burst the TDMA
 * timeslot / frame / multiframe, per CRC-good block the headers of its MAC PDUs, as small int32
 * records (k_etsi_mac, one launch).  Stands in for the header dissection of the reference's
 * TetraProtocolParser.parse_mac_pdu (/root/reference/tetraear/core/protocol.py:349-596) on
 * channel-decoded SCH/F, SCH/HD and BSCH type-1 blocks, whose layout (EN 300 392-2 §21.4) that
 * parser's raw-frame layout does not fit; tetra_mac_headers above keeps the reference's own layout
 * for the compat chain.  The SYNC PDU and the TDMA timebase have no reference counterpart.  The
 * field layouts are transcribed from EN 300 392-2 §21.4 / §18.4.2 and not pinned against a
 * conformance vector; the records carry raw fields.
 *
 * Inputs: the outputs of tetra_lmac_etsi / _acquire / _stream (host or device) and that call's
 * nsym.  Nothing past nburst[c] / nblock[c] (clamped to MAXB / MAXJ) or past a block's type-1
 * length is read.  A type-1 bit is byte & 1, bit 0 the block's first, fields MSB first.
 *
 * pdus [C][MAXJ][MAXPDU][16]: the walk of a CRC-good block of n1 bits.  BSCH: one SYNC record.
 * SCH: from off = 0, while n1 - off >= 16, parse and count the PDU at off; stop after a null PDU,
 * FRAG, a broadcast or supplementary PDU, L = 62 / 63 or STATUS 1, else off += 8 L.  npdu [C][MAXJ]
 * (fully written) counts them, 0 for a CRC-bad block and for j >= nblock[c]; the first MAXPDU are
 * recorded, records past the count are not written.  Length indication L: 2..34 octets (8 L may run
 * past the block end by fewer than 8 bits: cut there), 62 / 63 the rest of the block, else malformed.
 *
 * slots [C][MAXB][TETRA_SLOT_FIELDS] (rows past nburst[c] not written) and tdma [C] (in/out): the
 * timebase, bursts in order, p = bit0 + start bit (int64):
 *   1. an SB whose BSCH block is CRC-good with a STATUS 0 SYNC record: slot from its TN/FN/MN,
 *      FLAGS bit 0 (bit 1: the channel was locked and rule 2 gave another slot or none); anchor =
 *      (p, slot), locked;
 *   2. else when locked: d = p - anchor_bit, k = (d + 255) / 510, r = d - 510 k; d < 0 or
 *      k >= TETRA_TDMA_EXPIRE drops the lock (rule 3); |r| <= TETRA_TDMA_TOL: slot = (anchor_slot
 *      + k) % TETRA_TDMA_SLOTS and the anchor moves to (p, slot); else unknown, anchor kept;
 *   3. unlocked or unknown: the row reads 0, 0, 0, 0.
 * After the last burst bit0 += 2 max(nsym[c] - 1, 0).
 * With device pointers the call enqueues on the context stream and returns without waiting. */
#define TETRA_ETSI_MAXPDU 4
#define TETRA_TDMA_SLOTS 4320          /* 60 multiframes x 18 frames x 4 slots */
#define TETRA_TDMA_TOL 4               /* bits a burst may sit off the slot grid */
#define TETRA_TDMA_EXPIRE 72           /* slots without a burst after which the timebase is dropped */
typedef struct tetra_etsi_tdma {       /* per channel, carried from chunk to chunk; all zero = new stream */
    int64_t bit0;                      /* stream bit index of this chunk's first new dibit */
    int64_t anchor_bit;                /* stream bit of the last burst placed on the slot grid */
    int32_t anchor_slot;               /* its slot count ((MN-1)*18 + (FN-1))*4 + TN field, 0..4319 */
    int32_t locked;
} tetra_etsi_tdma;
enum { TETRA_SLOT_TN = 0, TETRA_SLOT_FN, TETRA_SLOT_MN, TETRA_SLOT_FLAGS, TETRA_SLOT_FIELDS = 4 };
/* TN 1..4, FN 1..18, MN 1..60, all 0 = unknown.
 * FLAGS bit 0: set from this burst's own SYNC PDU; bit 1: that PDU disagreed with the prediction */
/* PDU record fields common to every kind */
enum {
    TETRA_PDU_KIND = 0,     /* TETRA_PDU_* below */
    TETRA_PDU_OFFSET,       /* first bit of the PDU in the block */
    TETRA_PDU_NBITS,        /* bits the PDU occupies */
    TETRA_PDU_STATUS,       /* 0 ok; 1 malformed or truncated: a bad L, a header or SYSINFO body past the PDU
                               or block end, a SYNC with FN outside 1..18 or MN outside 1..60 */
    /* RESOURCE, FRAG, END, null (a field a kind does not have reads 0; SSI and AUX read -1) */
    TETRA_PDU_FILL = 4,     /* fill-bit indication */
    TETRA_PDU_ENC,          /* encryption mode */
    TETRA_PDU_LENGTH,       /* raw L */
    TETRA_PDU_ADDR_TYPE,    /* 0 null, 1 SSI, 2 event label, 3 USSI, 4 SMI, 5 SSI + event label,
                               6 SSI + usage marker, 7 SMI + event label */
    TETRA_PDU_SSI,          /* the 24-bit SSI, USSI or SMI */
    TETRA_PDU_AUX,          /* event label (10 bits) or usage marker (6) */
    TETRA_PDU_HDR_BITS,     /* bit within the PDU after the parsed header (where the optional
                               elements begin): RESOURCE 16 + address, END 11, FRAG 4 */
    TETRA_PDU_FLAGS,        /* bit 0 position of grant, bit 1 random access flag */
    TETRA_PDU_FIELDS = 16
    /* SYNC 4..15: system code, colour code, TN field, FN, MN, sharing mode, TS reserved frames, flags
     *   (bit 0 U-plane DTX, bit 1 frame-18 extension, bit 2 late entry), MCC, MNC, neighbour cell
     *   broadcast, cell service level.
     * SYSINFO 4..15: main carrier, band, offset, duplex spacing, reverse operation, number of common
     *   secondary control channels, MS_TXPWR_MAX_CELL, RXLEV_ACCESS_MIN, ACCESS_PARAMETER |
     *   RADIO_DOWNLINK_TIMEOUT << 4 | optional field flag << 8, hyperframe/CCK flag << 16 | its 16-bit
     *   value, location area, subscriber class | BS service details << 16 (a SYSINFO whose 124 bits
     *   do not fit the block: STATUS 1, fields 0).
     * ACCESS-DEFINE, other broadcast, supplementary: 4..15 read 0. */
};
enum {
    TETRA_PDU_RESOURCE = 0, TETRA_PDU_FRAG, TETRA_PDU_END, TETRA_PDU_SYSINFO, TETRA_PDU_ACCESS_DEFINE,
    TETRA_PDU_BROADCAST, TETRA_PDU_SUPPL, TETRA_PDU_SYNC, TETRA_PDU_NULL
};
int tetra_etsi_mac(tetra_ctx *ctx, const int32_t *nsym, size_t C, const int32_t *nburst, const int32_t *bursts,
                   const int32_t *nblock, const int32_t *blocks, const uint8_t *type1, tetra_etsi_tdma *tdma,
                   int32_t *slots /*[C][MAXB][4]*/, int32_t *npdu /*[C][MAXJ]*/,
                   int32_t *pdus /*[C][MAXJ][MAXPDU][16]*/);
/* tetra_etsi_mac over groups of overlapping rows (a new symbol of ABI version 2; nothing existing
 * changed shape).  Rows g G .. g G + G - 1 are the chunk rows of carrier g in time order, as for
 * tetra_lmac_etsi_acquire_groups; row i of a group starts row_bits bits after row i - 1 (the wideband
 * chain: m2 / 2), so consecutive rows may share bursts.  npdu and pdus are tetra_etsi_mac's.  Per
 * group, the live bursts (row i, burst b < nburst clamped to 0..MAXB) have pos = i row_bits + start
 * bit (int64) and are taken in the order (pos, row, b):
 *   keep [C][MAXB]: 1 for the first burst of the order and for every burst whose pos exceeds that of
 *     the previous burst in the order (kept or not) by more than tol_bits, else 0 -- each burst
 *     once, the first copy; rows past nburst not written;
 *   slots [C][MAXB][TETRA_SLOT_FIELDS] and tdma [C / G] (in/out): one timebase per group over all
 *     live bursts in that order, p = bit0 + pos:
 *     1. when locked: d = p - anchor_bit, k = floor((d + 255) / 510), r = d - 510 k.  k >=
 *        TETRA_TDMA_EXPIRE drops the lock; k <= -TETRA_TDMA_EXPIRE predicts nothing and keeps it;
 *        else |r| <= TETRA_TDMA_TOL predicts slot (anchor_slot + k) mod TETRA_TDMA_SLOTS.  d < 0
 *        does not drop the lock: a burst's copy in the next row, and every burst of a carried tail,
 *        sits behind the anchor;
 *     2. an SB with its own STATUS 0 SYNC (as tetra_etsi_mac's rule 1): its slot, FLAGS bit 0, bit 1
 *        if the group was locked on entry to this burst and rule 1 predicted another slot or none;
 *        anchor = (p, slot), locked -- also when p is behind the anchor;
 *     3. else a predicted burst takes that slot, and the anchor moves to (p, slot) only if k >= 1;
 *     4. else the row reads 0, 0, 0, 0.
 *     After the walk bit0 += advance.  Rows past nburst are not written.
 * 1 <= G <= 64, C % G == 0, row_bits >= 0 and tol_bits >= 0, else TETRA_E_INVALID with nothing
 * written.  G = 1 on rows of ascending start bits (at least 256 bits apart) with row_bits = 0 and
 * advance = 2 max(nsym - 1, 0) equals tetra_etsi_mac.  nsym [C] is not read.  Host or device pointers. */
int tetra_etsi_mac_groups(tetra_ctx *ctx, const int32_t *nsym, size_t C, size_t G, int64_t row_bits,
                          int64_t tol_bits, int64_t advance, const int32_t *nburst, const int32_t *bursts,
                          const int32_t *nblock, const int32_t *blocks, const uint8_t *type1,
                          tetra_etsi_tdma *tdma /*[C/G] in/out*/, int32_t *keep /*[C][MAXB]*/,
                          int32_t *slots /*[C][MAXB][4]*/, int32_t *npdu /*[C][MAXJ]*/,
                          int32_t *pdus /*[C][MAXJ][MAXPDU][16]*/);

/* Link quality of the ETSI chain's bursts and blocks (a new symbol of ABI version 2; nothing existing
 * changed shape): how many channel bits the decoder corrected in a block, how many known bits of a
 * burst were wrong, how strong the soft bits were.  It stands in for the signal-quality read-out of
 * the reference's capture loop; on decoded blocks the reference has no counterpart.  All exact
 * integers, restated in tests/_etsi_quality_model.py.
 *
 * Inputs: the rows softbits [C][2 stride] / hard [C][stride] a lower-MAC call read, still intact, and
 * that call's outputs.  origin_bits: the row bit the start bits count from -- 0 for tetra_lmac_etsi,
 * _acquire and _acquire_groups, 2 * TETRA_ETSI_RESERVE for tetra_lmac_etsi_stream (whose start bits may
 * be negative; stream into next rows other than the input rows, or the rows read are gone).
 * cell_init [C / G]: the scrambling init rows g G .. g G + G - 1 were descrambled with (the
 * configured init, or the value the acquire call returned); the sequences are formed on the device
 * from it, whatever the context's cell table holds.
 *
 * bq [C][MAXB][TETRA_LQ_FIELDS], for b < nburst[c] (clamped to 0..MAXB; nothing past it written).  A
 * burst is invalid when its kind is outside 0..2 or row bits origin_bits + start .. + 510 do not lie
 * inside the row's 2 stride bits: nothing of it is read and it reads -1, -1, -1, -1.  Else, a hard
 * bit at row bit p being hard[c][p >> 1] bit (p & 1 ? 0 : 1) and every position relative to
 * origin_bits + start: TERR the training bits that differ from the kind's sequence (22 at 244 for
 * n / p, 38 at 214 for y), HERR the differing bits among the 12 head bits at 0 and the 10 tail bits
 * at 500, WSUM the sum of |soft| over the 510 bits (|-128| = 128), NSAT those with |soft| >= 127.
 *
 * kq [C][MAXJ][TETRA_LQ_FIELDS], for j < nblock[c] (clamped likewise).  Block j of kind k (K = 432 /
 * 216 / 120 coded bits) lies at offset 282 of its burst for block index 1, else 14 (SCH/F, SCH/HD)
 * or 94 (BSCH); SCH/F's coded bits from 216 on lie 52 bits further.  A CRC-bad block reads -1, 0, 0,
 * 0.  A block of an invalid burst -- or one that names no live burst, a kind outside 0..2, or a
 * block index its kind does not have -- reads -1, -1, -1, -1.  Else its type-1 bits (byte & 1) are
 * encoded as by tetra_etsi_encode_blocks (BSCH with scrambler init 3, else the row's cell) into
 * c_0 .. c_K-1 and compared with the soft values s_i at those row bits: NERR the positions with
 * s_i != 0 and (s_i < 0) != (c_i == 1), WERR the sum of |s_i| over them, WSUM the sum of |s_i| over
 * all K, NZERO the positions with s_i == 0.
 *
 * C == 0, stride == 0, G == 0, C % G != 0, origin_bits < 0 or a NULL array: TETRA_E_INVALID, nothing
 * written.  Host or device pointers; with device pointers the call enqueues one kernel on the context
 * stream and returns without waiting (no allocation, no synchronising copy). */
enum { TETRA_LQ_NERR = 0, TETRA_LQ_WERR, TETRA_LQ_WSUM, TETRA_LQ_NZERO, TETRA_LQ_FIELDS = 4 };
enum { TETRA_BQ_TERR = 0, TETRA_BQ_HERR, TETRA_BQ_WSUM, TETRA_BQ_NSAT };
int tetra_etsi_link_quality(tetra_ctx *ctx, const int8_t *softbits, const uint8_t *hard, size_t C, size_t stride,
                            int32_t origin_bits, size_t G, const uint32_t *cell_init /*[C/G]*/,
                            const int32_t *nburst, const int32_t *bursts, const int32_t *nblock,
                            const int32_t *blocks, const uint8_t *type1,
                            int32_t *bq /*[C][MAXB][4]*/, int32_t *kq /*[C][MAXJ][4]*/);

/* ---------------------------------------------------------------- timebase vote (a new symbol of ABI
 * version 2; nothing existing changed shape).  tetra_etsi_mac_groups takes every STATUS 0 SYNC at its
 * word: one false CRC pass on a BSCH (2^-16 per failed block, its TN / FN / MN valid about half the
 * time) or a neighbour cell's synchronisation burst re-anchors the carrier's slot grid, and it keeps
 * the copy of a burst in the earlier row whatever that copy decoded.  tetra_etsi_mac_vote_groups is that
 * call with the timebase chosen by a vote and keep chosen by quality, from the records of
 * tetra_etsi_link_quality for the same rows and the same lower-MAC outputs (bq, kq).  npdu and pdus are
 * tetra_etsi_mac's.
 *
 * The rule (exact integers, positions int64).
 *   Order.  A group's live bursts (row i, b < nburst clamped to 0..MAXB) have pos = i row_bits + start
 *     bit and are taken in the order (pos, row, b), as in tetra_etsi_mac_groups.
 *   Clusters.  A cluster is a maximal run of that order in which every burst's pos exceeds the previous
 *     burst's by at most tol_bits (the chain rule); its first burst is what tetra_etsi_mac_groups keeps.
 *   Keep.  Burst (c, b) has a quality key Q.  good = the number of j < nblock[c] (clamped to 0..MAXJ)
 *     with blocks[c][j] naming burst b, a kind in 0..2 and crc_ok != 0.  bq[c][b][TERR] < 0 (an invalid
 *     burst): Q = -1.  Else Q = good << 32 | (60 - min(60, TERR + HERR)) << 16 | min(WSUM, 65535), with
 *     TERR, HERR, WSUM from bq (a negative sum or WSUM, which no record has, reads as 0).  In every
 *     cluster exactly one burst has keep = 1: the one with the largest Q, on a tie the first in the order.
 *   Ballots.  A burst has an own SYNC as in tetra_etsi_mac_groups: an SB whose BSCH block is CRC-good
 *     with a STATUS 0 record, of slot count s.  Its weight is w = max(1, WSUM - 2 WERR) from that block's
 *     kq record -- the cell vote's w, at most 15240 (a larger value, which no record has, reads as
 *     15240); a kq record whose NERR reads -1 gives w = 1.  In every cluster the own-SYNC burst with the
 *     largest w (on a tie the first) is the cluster's ballot, cast where the walk reaches it; every other
 *     burst of the cluster is walked as a burst without a SYNC: one burst on air casts one ballot.
 *   The walk.  One per group over all live bursts in the order, kept or not, p = bit0 + pos.  State:
 *     tdma[g] and score = max(0, tscore[g]).  Rule 1 of tetra_etsi_mac_groups gives (pred, k); a lock
 *     that expires (k >= TETRA_TDMA_EXPIRE) also sets score to 0.  For a ballot (s, w):
 *       a. not locked: anchor = (p, s), locked, score = min(cap, w); the row is s, FLAGS 1; BALLOTS++;
 *       b. locked and pred == s: score = min(cap, score + w), anchor = (p, s); the row is s, FLAGS 1;
 *          BALLOTS++, AGREED++;
 *       c. locked and pred != s (another slot, or none): if w > score the ballot wins: anchor = (p, s),
 *          score = min(cap, w - score); the row is s, FLAGS 1 | 2; BALLOTS++, WON++.  Otherwise score -=
 *          w; if pred is a slot the burst takes it with FLAGS 2 | 4 (bit 2: own SYNC outvoted) and the
 *          anchor moves to (p, pred) only if k >= 1; if pred is none the row reads 0, 0, 0, 0;
 *          BALLOTS++, OUTVOTED++.
 *     Every other burst follows rules 3 and 4 of tetra_etsi_mac_groups.  After the walk bit0 += advance
 *     and tscore[g] = score; without a ballot tscore changes only by expiry (and a negative one to 0).
 * tvote [C / G][TETRA_TV_FIELDS] (fully written): the group's ballots of this call and how they fared.
 *
 * On an input where no cluster holds two own-SYNC bursts and tetra_etsi_mac_groups sets FLAGS bit 1
 * nowhere, slots and tdma equal tetra_etsi_mac_groups's from any incoming score, and keep equals it
 * wherever a cluster's copies have equal Q.  (An SB that arrives as the lock expires reads FLAGS 1 here,
 * case a, and FLAGS 3 there.)  Why a cap this small is safe: a stream that really restarted on another
 * bit alignment places no burst on the old grid, so the lock expires by itself after TETRA_TDMA_EXPIRE
 * slots and the next SYNC starts from score 0; the cap only bounds how long a grid that happens to share
 * the alignment defends its slot numbers.  TETRA_TDMA_VOTE_CAP_DEFAULT: four full-scale BSCH blocks, a
 * stated choice, not a measurement.
 *
 * TETRA_E_INVALID with nothing written: what tetra_etsi_mac_groups refuses, a NULL array, cap <= 0.
 * Host or device pointers; with device pointers the call enqueues two kernels on the context stream and
 * returns without waiting (no allocation, no synchronising copy).  struct tetra_etsi_tdma is unchanged:
 * the score lives in its own array. */
#define TETRA_TDMA_VOTE_CAP_DEFAULT 60960
enum { TETRA_TV_BALLOTS = 0, TETRA_TV_AGREED, TETRA_TV_OUTVOTED, TETRA_TV_WON, TETRA_TV_FIELDS = 4 };
int tetra_etsi_mac_vote_groups(tetra_ctx *ctx, const int32_t *nsym, size_t C, size_t G, int64_t row_bits,
                               int64_t tol_bits, int64_t advance, int32_t cap,
                               const int32_t *nburst, const int32_t *bursts, const int32_t *nblock,
                               const int32_t *blocks, const uint8_t *type1,
                               const int32_t *bq /*[C][MAXB][4] in*/, const int32_t *kq /*[C][MAXJ][4] in*/,
                               tetra_etsi_tdma *tdma /*[C/G] in/out*/, int32_t *tscore /*[C/G] in/out*/,
                               int32_t *keep, int32_t *slots, int32_t *npdu, int32_t *pdus,
                               int32_t *tvote /*[C/G][TETRA_TV_FIELDS] out*/);

/* ---------------------------------------------------------------- traffic slots (a new symbol of ABI
 * version 2; nothing existing changed shape).  The reference's capture loop builds the speech codec's
 * input from every frame that looks like traffic (_extract_voice_slot_from_symbols); the ETSI chain
 * reported such a slot only as "SCH/F, CRC bad".  tetra_etsi_traffic classifies every burst of a
 * lower-MAC call and copies out, for the bursts the control decoders could not read, what the speech
 * codec's own channel decoder consumes: the block fields' type-4 soft bits, i.e. descrambled with the
 * cell's sequence and nothing more (TCH is exported, not decoded).  All exact integers, restated in
 * tests/_etsi_traffic_model.py.
 *
 * Inputs: those of tetra_etsi_link_quality, with the same meaning of origin_bits, G and cell_init; the
 * rows must be the ones the lower-MAC call read, still intact.  slots [C][MAXB][TETRA_SLOT_FIELDS] and
 * keep [C][MAXB] are the outputs of tetra_etsi_mac / _groups / _vote_groups for the same rows, or NULL.
 *
 * tq [C][MAXB][TETRA_TQ_FIELDS] and tch [C][MAXB][TETRA_TCH_BITS], for b < nburst[c] (clamped to
 * 0..MAXB; nothing past it written in either).  The first of these that applies decides CLASS:
 *   a. an invalid burst (kind outside 0..2, or row bits origin_bits + start .. + 510 not inside the
 *      row's 2 stride bits): nothing of it is read, tq reads -1, -1, -1, -1, tch is not written;
 *   b. keep != NULL and keep[c][b] == 0 (the copy not chosen): NONE;
 *   c. kind 2 (synchronisation burst): NONE;
 *   d. slots != NULL and slots[c][b][TETRA_SLOT_FN] == 18 (the control frame): CONTROL;
 *   e. kind 0: CONTROL if some j < nblock[c] (clamped to 0..MAXJ) has blocks[c][j] == (kind 0,
 *      crc_ok != 0, burst b, index 0), otherwise FULL;
 *   f. kind 1, with g0 / g1 the same test for (kind 1, index 0) / (kind 1, index 1): both CONTROL, g0
 *      only HALF (the first half was stolen and decoded, the second is a traffic half slot), otherwise
 *      LOST.
 * NONE, CONTROL and LOST set NBITS, WSUM and NZERO to 0 and leave tch unwritten.  FULL exports n = 432
 * values, s_i the soft byte at burst bit 14 + i for i < 216 and at 282 + (i - 216) from there on; HALF
 * n = 216, s_i at burst bit 282 + i.  With q_i bit i of the scrambling sequence of cell_init[c / G]
 * (every block is scrambled from the sequence's start), tch[c][b][i] = q_i ? (s_i == -128 ? 127 : -s_i)
 * : s_i for i < n; bytes from n on are not written.  NBITS = n, WSUM = the sum of |tch_i| (|-128| =
 * 128), NZERO = the count of tch_i == 0.  The chain's sign convention is kept: positive means bit 0.
 *
 * Without the AACH a FULL slot is a candidate: a control burst lost to noise looks the same.  WSUM and
 * the timebase are what a caller gates on; tetra_etsi_assign (below) adds what the control channel
 * announced about the carrier and timeslot.
 *
 * C == 0, stride == 0, G == 0, C % G != 0, origin_bits < 0 or a NULL required array: TETRA_E_INVALID,
 * nothing written.  Host or device pointers; with device pointers the call enqueues one kernel on the
 * context stream and returns without waiting (no allocation, no synchronising copy). */
enum { TETRA_TQ_CLASS = 0, TETRA_TQ_NBITS, TETRA_TQ_WSUM, TETRA_TQ_NZERO, TETRA_TQ_FIELDS = 4 };
enum { TETRA_TCH_NONE = 0, TETRA_TCH_CONTROL, TETRA_TCH_FULL, TETRA_TCH_HALF, TETRA_TCH_LOST };
#define TETRA_TCH_BITS 432
int tetra_etsi_traffic(tetra_ctx *ctx, const int8_t *softbits, size_t C, size_t stride, int32_t origin_bits,
                       size_t G, const uint32_t *cell_init /*[C/G]*/,
                       const int32_t *nburst, const int32_t *bursts, const int32_t *nblock, const int32_t *blocks,
                       const int32_t *slots /*[C][MAXB][4] or NULL*/, const int32_t *keep /*[C][MAXB] or NULL*/,
                       int32_t *tq /*[C][MAXB][4]*/, int8_t *tch /*[C][MAXB][432]*/);

/* TM-SDUs and fragment reassembly (a new symbol of ABI version 2; nothing existing changed shape):
 * where the TM-SDU of every recorded MAC-RESOURCE / MAC-FRAG / MAC-END PDU lies, its bytes, and the
 * fragments of a carrier joined across bursts, chunks and overlapping rows into whole TM-SDUs -- what
 * an upper MAC consumes (the reference's MacPDU.data / reassembled_data, protocol.py:560-596, which
 * keeps one fragment buffer that every MAC-RESOURCE overwrites).  It runs after tetra_etsi_mac /
 * _groups / _vote_groups on their npdu / pdus (and keep) and on the type1 rows they read.  All exact
 * integers, restated in tests/_etsi_sdu_model.py.  The element layouts below are transcribed from EN
 * 300 392-2 §21.4.3 / §21.5.2 and not pinned against a conformance vector; the
 * records carry the raw fields, so a correction is a change to this table and the model's.
 *
 * Part A, per recorded PDU q < min(npdu[c][j], MAXPDU) of block j < nblock[c] (clamped) with crc_ok != 0
 * and block kind SCH/F, SCH/HD or BSCH: sdu [C][MAXJ][MAXPDU][TETRA_SDU_FIELDS].  Records past that
 * count, and records of blocks with npdu == 0, CRC-bad blocks and j >= nblock[c], are not written.
 * With off = PDU OFFSET, end = off + PDU NBITS, the optional elements begin at off + HDR_BITS:
 *   MAC-RESOURCE  power control flag 1 [+ power control 4]; slot granting flag 1 [+ slot granting 8];
 *                 channel allocation flag 1 [+ body]
 *   MAC-END       slot granting flag 1 [+ slot granting 8]; channel allocation flag 1 [+ body]
 *   MAC-FRAG      none
 *   channel allocation body: allocation type 2, timeslot assigned 4, up/downlink assigned 2, CLCH
 *                 permission 1, cell change flag 1, carrier number 12, extended carrier numbering flag 1
 *                 [+ band 4, offset 2, duplex spacing 3, reverse operation 1], monitoring pattern 2
 *                 [+ frame-18 monitoring pattern 2 if monitoring pattern == 0]
 * Up/downlink assigned == 0 is the augmented form: not walked, STATUS 4.  The TM-SDU runs from the end
 * of the elements to end; with the fill-bit indication set, the last 1 bit before end (at or behind
 * the elements' end) and the zeros after it are fill, and the SDU ends before that 1.  0 bits is valid.
 *   STATUS       0 ok.  1 none: a kind without a TM-SDU (SYNC, broadcast, supplementary), a null PDU, or
 *                PDU STATUS != 0.  2 malformed: an element runs past end, the fill flag is set and no 1
 *                lies behind the elements, or the PDU record itself does not lie inside the block.  3
 *                encrypted: a MAC-RESOURCE with ENC != 0; elements are not interpreted, the exported bits
 *                are the PDU's from off + HDR_BITS to end, untouched.  4 unsupported.
 *   OFFSET,NBITS first TM-SDU bit in the block and its length (0, 0 unless STATUS is 0 or 3)
 *   BYTE         byte offset of this SDU in the block's sdu_data row (the running sum of the earlier
 *                SDUs' (NBITS + 7) / 8; written for every record)
 *   ROLE         by kind, whatever the status: 1 first fragment (MAC-RESOURCE with L == 63), 2 middle
 *                (MAC-FRAG), 3 last (MAC-END), else 0 (whole, or none)
 *   ELEMS        bit 0 power control present, bit 1 slot granting, bit 2 channel allocation, bit 3 the
 *                extended carrier numbering fields
 *   POWER_GRANT  power control | slot granting << 8 | the 10 extended carrier bits << 16
 *   CHAN         the 10 bits allocation type .. cell change flag | frame-18 monitoring pattern << 10 |
 *                carrier number << 16 | monitoring pattern << 28
 *   A walk that stops (STATUS 2 or 4) keeps in ELEMS / POWER_GRANT / CHAN what it read before; a value
 *   is read whole or not at all, and so are the ten bits allocation type .. cell change flag and the ten
 *   extended carrier bits.
 * sdu_data [C][MAXJ][TETRA_SDU_ROW]: the (NBITS + 7) / 8 bytes of every STATUS 0 / 3 SDU at BYTE, MSB
 * first, the last byte zero-padded; bytes not covered by an SDU are not written.
 *
 * Part B, per group of G rows (tetra_etsi_mac_groups' grouping: row i of a group starts row_bits after
 * row i - 1, the live bursts in the order (pos, row, b), pos = i row_bits + start bit): frag [C / G]
 * (in/out; all zero = a new stream) joins the fragments.  keep [C][MAXB] NULL means every burst; where
 * given, a burst with keep == 0 is skipped.  G == 1, row_bits == 0 and keep == NULL is the streaming form:
 * bit0 advances by 2 max(nsym[c] - 1, 0) (nsym required); otherwise by `advance` (nsym not read).
 * The walk visits the kept bursts in order, p = bit0 + pos; of each burst the blocks j ascending with
 * blocks[c][j] burst index == b that Part A wrote records for; of each block its recorded PDUs in order.
 * With, for a chain, d = p - last_bit, k = floor((d + 255) / 510):
 *   1. Expiry.  Before each kept burst every active chain with k > gap_slots is freed, dropped += 1.
 *   2. Same timeslot: k >= 0, k % 4 == 0 and |d - 510 k| <= TETRA_TDMA_TOL (k == 0: the same burst).
 *   3. ROLE 1, STATUS 0: every active chain on the same timeslot is freed (superseded), dropped += 1
 *      each; the lowest free chain is taken, else the chain with the smallest last_bit (the lowest index
 *      among equals) is evicted, dropped += 1.  It starts with the SDU's bits: ssi / addr_type / aux /
 *      enc of the PDU, nfrag = fed = 1, span = 0, last_bit = p.
 *   4. ROLE 2 or 3, STATUS 0: the lowest active chain on the same timeslot takes the bits, appended at
 *      its bit length; none: orphans += 1.  If nbits would exceed 8 TETRA_SDU_MAXBYTES the chain is freed,
 *      dropped += 1, and nothing more happens.  Else nfrag += 1, span += k, fed += (k > 0), last_bit = p;
 *      a ROLE 3 then writes a done record and frees the chain.
 *   5. ROLE 1 with STATUS != 0 starts nothing; ROLE 2 / 3 with STATUS != 0 is an orphan.  ROLE 0: nothing.
 *   6. After the walk bit0 advances.
 * ndone [C / G] (fully written) counts the completions of the call; the first maxd are recorded in done
 * [C / G][maxd][TETRA_DONE_FIELDS] with the (NBITS + 7) / 8 bytes in done_data [C / G][maxd]
 * [TETRA_SDU_MAXBYTES]; the rest, and bytes past a message's, are not written (maxd == 0: done and
 * done_data may be NULL).  ROW is the row c of the call, BURST / BLOCK (j) / PDU where the MAC-END sat;
 * GAPS = SPAN / 4 + 1 - FED, the same-timeslot slots between the first and last feed that fed nothing:
 * 0 means no fragment can have been lost.
 *
 * C == 0, a NULL required array, G outside 1..64, C % G != 0, row_bits, gap_slots or maxd < 0, C > 2^24:
 * TETRA_E_INVALID, nothing written.  Host or device pointers; with device pointers the call enqueues two
 * kernels on the context stream and returns without waiting. */
#define TETRA_SDU_ROW 40            /* 268 bits plus at most 7 pad bits for each of 4 PDUs */
#define TETRA_SDU_MAXBYTES 512      /* a chain's longest TM-SDU (unpinned: overflow drops the chain) */
#define TETRA_FRAG_CHAINS 4         /* a carrier has four timeslots */
enum {
    TETRA_SDU_STATUS = 0, TETRA_SDU_OFFSET, TETRA_SDU_NBITS, TETRA_SDU_BYTE, TETRA_SDU_ROLE, TETRA_SDU_ELEMS,
    TETRA_SDU_POWER_GRANT, TETRA_SDU_CHAN, TETRA_SDU_FIELDS = 8
};
enum { TETRA_SDU_OK = 0, TETRA_SDU_NONE, TETRA_SDU_MALFORMED, TETRA_SDU_ENCRYPTED, TETRA_SDU_UNSUPPORTED };
enum { TETRA_ROLE_WHOLE = 0, TETRA_ROLE_FIRST, TETRA_ROLE_MIDDLE, TETRA_ROLE_LAST };
enum {
    TETRA_DONE_ROW = 0, TETRA_DONE_BURST, TETRA_DONE_BLOCK, TETRA_DONE_PDU, TETRA_DONE_SSI, TETRA_DONE_ADDR_TYPE,
    TETRA_DONE_AUX, TETRA_DONE_ENC, TETRA_DONE_NBITS, TETRA_DONE_NFRAG, TETRA_DONE_SPAN, TETRA_DONE_FED,
    TETRA_DONE_GAPS, TETRA_DONE_FIELDS = 13
};
typedef struct tetra_etsi_frag_chain {
    int64_t last_bit;                  /* stream bit of the burst that fed it last */
    int32_t active;
    int32_t ssi, addr_type, aux, enc;  /* of the starting PDU */
    int32_t nbits, nfrag;
    int32_t span;                      /* slots from the first feed to the last */
    int32_t fed;                       /* distinct bursts that fed it */
    int32_t reserved;
    uint8_t data[TETRA_SDU_MAXBYTES];  /* MSB first, zero behind nbits in its last byte */
} tetra_etsi_frag_chain;
typedef struct tetra_etsi_frag {       /* per carrier, carried from call to call; all zero = new stream */
    int64_t bit0;                      /* stream bit index of this call's position 0 */
    int32_t dropped;                   /* chains freed unfinished: expired, superseded, evicted, overflowed */
    int32_t orphans;                   /* middle / last fragments that found no chain */
    tetra_etsi_frag_chain chain[TETRA_FRAG_CHAINS];
} tetra_etsi_frag;
int tetra_etsi_sdu(tetra_ctx *ctx, const int32_t *nsym, size_t C, size_t G, int64_t row_bits, int64_t advance,
                   int32_t gap_slots, const int32_t *nburst, const int32_t *bursts, const int32_t *nblock,
                   const int32_t *blocks, const uint8_t *type1, const int32_t *npdu, const int32_t *pdus,
                   const int32_t *keep /*[C][MAXB] or NULL*/, int32_t *sdu /*[C][MAXJ][MAXPDU][8]*/,
                   uint8_t *sdu_data /*[C][MAXJ][40]*/, tetra_etsi_frag *frag /*[C/G] in/out*/, int32_t maxd,
                   int32_t *ndone /*[C/G]*/, int32_t *done /*[C/G][maxd][13]*/,
                   uint8_t *done_data /*[C/G][maxd][512]*/);

/* LLC headers, the frame check sequence and TL-SDUs (a new symbol of ABI version 2; nothing existing
 * changed shape): a TM-SDU is an LLC PDU -- a 4-bit type, the basic link's sequence bits, the TL-SDU and,
 * for half the types, a 32-bit FCS, the only end-to-end check a reassembled message has.  The call runs
 * after tetra_etsi_sdu on that call's outputs (nblock / blocks / npdu / pdus as given to it; sdu, sdu_data,
 * ndone, done, done_data as it left them) and writes one record per TM-SDU plus the TL-SDU byte-aligned.
 * All exact integers, restated in tests/_etsi_llc_model.py.
 *
 * Pinned: the CRC arithmetic below (b"123456789" gives 0xFC891918; the register run on over a message's
 * own FCS leaves 0xC704DD7B; for whole bytes the value is bitrev32(zlib.crc32(bytes(bitrev8(x) for x in
 * data)))).  Transcribed from EN 300 392-2 §21.2 and NOT pinned against a conformance vector (DESIGN.md
 * §5.25): that the FCS covers the LLC header, that it is sent most significant bit first, and the type
 * table.  FCS_RX and FCS_CALC are both recorded, so another convention can be tried on recorded data.
 *
 * Part A, llc [C][MAXJ][MAXPDU][TETRA_LLC_FIELDS] and tl [C][MAXJ][TETRA_SDU_ROW]: one record for every
 * record tetra_etsi_sdu's Part A writes (q < min(npdu[c][j], MAXPDU), j < nblock[c] clamped, crc_ok != 0,
 * block kind SCH/F, SCH/HD or BSCH); the rest is not written.  Part B, llc_done [C / G][maxd]
 * [TETRA_LLC_FIELDS] and tl_done [C / G][maxd][TETRA_SDU_MAXBYTES]: one record for each of the first
 * min(max(ndone[g], 0), maxd) done records of a group; the rest is not written (maxd == 0: done,
 * done_data, llc_done and tl_done may be NULL).
 *
 * The PDU's bits are the SDU's bytes from their first byte (sdu_data at BYTE, n = SDU NBITS bits; done_data,
 * n = DONE NBITS), MSB first.  STATUS, the first rule that holds:
 *   Part A  1 none       PDU KIND is not MAC-RESOURCE, or SDU ROLE != 0
 *           3 encrypted  SDU STATUS == 3 or PDU ENC != 0: nothing read, TYPE -1
 *           1 none       SDU STATUS 1, 2 or 4, or n <= 0
 *           2 malformed  BYTE < 0 or BYTE + (n + 7) / 8 > TETRA_SDU_ROW (no record of tetra_etsi_sdu's):
 *                        nothing read
 *   Part B  3 encrypted  DONE ENC != 0: nothing read, TYPE -1
 *           2 malformed  n < 0 or n > 8 TETRA_SDU_MAXBYTES: nothing read
 *           1 none       n == 0
 *   both    2 malformed  n < 4, or n < the type's header bits, plus 32 for a type with FCS
 *           4 unsupported  TYPE 8..15 (the advanced link, supplementary, layer-2 signalling): TYPE is
 *                        written, nothing else read
 *           0 ok
 *   TYPE      the first 4 bits: 0 BL-ADATA, 1 BL-DATA, 2 BL-UDATA, 3 BL-ACK, 4..7 the same four with FCS,
 *             8 AL-SETUP, 9 AL-DATA / AL-FINAL, 10 AL-UDATA / AL-UFINAL, 11 AL-ACK / AL-RNR, 12 AL-RECONNECT,
 *             13 supplementary, 14 layer-2 signalling, 15 AL-DISC
 *   NR, NS    the basic link's one-bit sequence numbers behind TYPE, -1 where the type has none: BL-ADATA
 *             N(R) then N(S) (header 6 bits), BL-DATA N(S) (5), BL-ACK N(R) (5), BL-UDATA neither (4)
 *   OFFSET    first TL-SDU bit in the SDU: the header's length, 4, 5 or 6
 *   NBITS     the TL-SDU's bits, n - OFFSET, less 32 for a type with FCS; 0 is valid (a bare BL-ACK)
 *   HEAD      the first min(NBITS, 8) bits of the TL-SDU left-aligned in 8 bits, -1 when NBITS < 3;
 *             HEAD >> 5 is the MLE protocol discriminator.  The device names nothing further.
 *   FCS       0 the type has none (FCS_RX and FCS_CALC then read 0), 1 good, 2 bad
 *   FCS_RX    the last 32 bits of the SDU, the first on air as bit 31 (the int32 holds the bit pattern)
 *   FCS_CALC  with r = 0xFFFFFFFF and, for each bit b of the PDU in front of the FCS, header included, in
 *             air order, t = (r >> 31) ^ b; r <<= 1; if (t) r ^= 0x04C11DB7: FCS_CALC = ~r.  Good iff
 *             FCS_CALC == FCS_RX.
 * With STATUS 1, 2, 3 or 4 every field not named in its row reads 0 (TYPE too on 1 and 2), NR and NS -1.
 * tl / tl_done: of every STATUS 0 record the (NBITS + 7) / 8 bytes of the TL-SDU, MSB first, the last byte
 * zero-padded -- in tl at the SDU's own BYTE offset in the block's row, in tl_done from byte 0; bytes not
 * covered are not written.
 *
 * C == 0, a NULL required array, G outside 1..64, C % G != 0, maxd < 0, C > 2^24: TETRA_E_INVALID, nothing
 * written.  Host or device pointers; with device pointers the call enqueues two kernels (one when maxd ==
 * 0) on the context stream and returns without waiting (no allocation, no synchronising copy). */
enum {
    TETRA_LLC_STATUS = 0, TETRA_LLC_TYPE, TETRA_LLC_NR, TETRA_LLC_NS, TETRA_LLC_OFFSET, TETRA_LLC_NBITS,
    TETRA_LLC_HEAD, TETRA_LLC_FCS, TETRA_LLC_FCS_RX, TETRA_LLC_FCS_CALC, TETRA_LLC_FIELDS = 10
};
enum { TETRA_LLC_OK = 0, TETRA_LLC_NONE, TETRA_LLC_MALFORMED, TETRA_LLC_ENCRYPTED, TETRA_LLC_UNSUPPORTED };
enum { TETRA_FCS_NONE = 0, TETRA_FCS_GOOD, TETRA_FCS_BAD };
int tetra_etsi_llc(tetra_ctx *ctx, size_t C, size_t G, const int32_t *nblock, const int32_t *blocks,
                   const int32_t *npdu, const int32_t *pdus, const int32_t *sdu /*[C][MAXJ][MAXPDU][8]*/,
                   const uint8_t *sdu_data /*[C][MAXJ][40]*/, int32_t maxd, const int32_t *ndone /*[C/G]*/,
                   const int32_t *done /*[C/G][maxd][13]*/, const uint8_t *done_data /*[C/G][maxd][512]*/,
                   int32_t *llc /*[C][MAXJ][MAXPDU][10]*/, uint8_t *tl /*[C][MAXJ][40]*/,
                   int32_t *llc_done /*[C/G][maxd][10]*/, uint8_t *tl_done /*[C/G][maxd][512]*/);

/* Channel allocations followed per carrier (a new symbol of ABI version 2; nothing existing changed
 * shape): the network announces traffic channels in clear on the control channel, and tetra_etsi_sdu
 * already reads the channel allocation element of every MAC-RESOURCE / MAC-END.  tetra_etsi_assign lists
 * those announcements with the carrier they name (Part A) and keeps, per carrier and timeslot, who was
 * assigned there and since when (Part B), so that a traffic candidate of tetra_etsi_traffic can be told
 * from noise by what the control channel said about it.  It runs after tetra_etsi_sdu on the same rows:
 * nburst / bursts / nblock / blocks / npdu / pdus / keep as given to it, sdu / ndone / done as it left
 * them, slots from the MAC call, tq from tetra_etsi_traffic.  All exact integers, restated in
 * tests/_etsi_assign_model.py.
 *
 * Transcribed from EN 300 392-2 and NOT pinned against a conformance vector: the carrier
 * numbering arithmetic below -- bands of 100 MHz, carriers of 25 kHz, the offsets 0 / +6.25 / -6.25 /
 * +12.5 kHz -- and the element layout of §5.24.  The records carry the raw fields, so a correction is a
 * change to this table and the model's.
 *
 * Geometry is tetra_etsi_sdu's: G rows a group (a carrier), row i of a group starting row_bits after row
 * i - 1, the live bursts (b < nburst clamped to 0..MAXB) in the order (pos, row, b), pos = i row_bits +
 * start bit, p = bit0 + pos (int64).  A burst is kept when keep is NULL or keep[c][b] != 0.  G == 1,
 * row_bits == 0 and keep == NULL is the streaming form: bit0 advances by 2 max(nsym[c] - 1, 0) (nsym
 * required); otherwise by `advance` (nsym not read).
 *
 * Carrier keys.  row_key [C / G] int32: the group's downlink carrier frequency in units of 6.25 kHz
 * (Hz / 6250); a negative key means unknown; row_key NULL means every key is -1.  Of a key >= 0, o = key &
 * 3 is its frequency offset in these units, 0 -> 0, 1 -> +1, 2 -> +2, 3 -> -1; base = key - offset, band =
 * base / 16000.  The target key of an allocation with carrier number n:
 *   ELEMS bit 3 clear   band 16000 + 4 n + offset, band and offset those of the carrier that sent it; -1 if
 *                       that carrier's key is unknown
 *   ELEMS bit 3 set     ext_band 16000 + 4 n + d, ext_band the 4-bit band and d from the 2-bit offset field
 *                       of the extended bits: 0 -> 0, 1 -> +1, 2 -> -1, 3 -> +2
 * Duplex spacing and reverse operation are carried in EXT and not used: only the downlink is followed.
 *
 * Part A, events.  nev [C / G] (fully written) counts a group's events; ev [C / G][maxe][TETRA_AE_FIELDS]
 * holds the first maxe in walk order, the rest is not written (maxe == 0: ev may be NULL).  The walk visits
 * the group's kept bursts in order; of each burst the blocks j < nblock[c] (clamped to 0..MAXJ) ascending
 * with blocks[c][j] burst index == b, crc_ok != 0 and kind SCH/F, SCH/HD or BSCH; of each block the PDUs q <
 * min(npdu[c][j], MAXPDU) ascending.  A PDU is an event when its sdu record has ELEMS bit 2 set and STATUS
 * == TETRA_SDU_OK and its PDU KIND is MAC-RESOURCE or MAC-END.  The record:
 *   ROW, BURST, BLOCK, PDU   c, b, j, q;  KIND the PDU kind
 *   HEAD        the 10 bits allocation type 2, timeslot assigned 4, up/downlink 2, CLCH 1, cell change 1
 *   CARRIER     the carrier number;  EXT the 10 extended bits, -1 without them;  TARGET the target key
 *   P_LO, P_HI  the burst's stream bit p, its low and high 32 bits
 *   TN, FN      of the burst's slots row; 0 when slots is NULL or the slot unknown
 *   SSI, ADDR_TYPE, AUX   a MAC-RESOURCE's own; a MAC-END's from the first of the group's first min(max(
 *               ndone[g], 0), maxd) done records whose ROW / BURST / BLOCK / PDU name it, -1 each if none
 *
 * Part B, the follower.  state [C / G] (in/out; all zero = a new stream) holds bit0, the counters expired
 * and released, and one entry per timeslot 1..4.  A recorded event (one of the first min(nev, maxe) of its
 * group) applies to target group t when TARGET == row_key[t] >= 0, its up/downlink field is 1 or 3
 * (downlink, or both), its timeslot bitmap is not 0, and t is the group that heard it or shared_clock != 0
 * -- the caller's promise that all groups count one sample clock, as the rows of a wideband capture do.
 * The time T of an event is its burst's p.  Per target group its applicable events, sorted by (T, source
 * group, ordinal in the source's list), and its own kept bursts, in their order, are merged by time: an
 * event at T is handled after every burst with p <= T and before every burst with p > T.
 *   Event.  For each timeslot n whose bit is set in the bitmap (its most significant bit is timeslot 1):
 *     an inactive entry becomes active with since = T, nalloc = 0, idle = 0; in every case last = T, nalloc
 *     += 1, and ssi / addr_type / aux / head become the event's SSI / ADDR_TYPE / AUX / HEAD, src_key the
 *     key of the carrier that sent it.
 *   Burst.  A kept burst takes part when slots gives its TN in 1..4 and, with tq given, its tq CLASS is
 *     not negative.  With d the entry of TN and slots_of(x) = floor((x + 255) / 510):
 *     1. if d is active and slots_of(p - last) > hold_slots it is freed, expired += 1;
 *     2. ta [C][MAXB][TETRA_TA_FIELDS] of the burst is written: STATE 1 if d is active, else 0; SSI,
 *        ADDR_TYPE, AUX, SRC_KEY, NALLOC, IDLE the entry's, AGE = slots_of(p - since) (its low 32 bits); an
 *        inactive entry reads SSI -1, ADDR_TYPE 0, AUX -1, SRC_KEY -1, NALLOC 0, IDLE 0, AGE 0;
 *     3. with tq given and d active: CLASS FULL or HALF sets idle = 0 and last = p; CLASS CONTROL on a
 *        burst whose FN is not 18 does idle += 1, and if then idle > idle_max the entry is freed, released
 *        += 1.
 *   Every other live burst -- not kept, TN unknown, slots NULL, or invalid for tetra_etsi_traffic -- reads
 *   STATE -1 and 0 in the other fields.  Rows past nburst are not written.  A freed entry keeps its other
 *   fields.  After the walk bit0 advances.
 *
 * Limits.  This follows announcements, it is not the AACH: without the AACH or CMCE's D-RELEASE nothing
 * announces the end of a call, so an allocation is kept alive by repeats (late-entry signalling) and by the
 * slot still looking like traffic, and ends when the slot visibly returns to decoded control signalling or
 * when neither was seen for hold_slots.  A carrier lost to noise reads FULL for ever and keeps its entry:
 * soft_sum, AGE and IDLE are what a caller gates on.  The augmented allocation (STATUS 4), uplink-only
 * allocations and encrypted PDUs are not followed.  TETRA_ASSIGN_HOLD_DEFAULT and TETRA_ASSIGN_IDLE_DEFAULT
 * are stated choices, not measurements.
 *
 * C == 0, G outside 1..64, C % G != 0, a NULL required array (every one but keep, slots, tq, row_key; nsym
 * in the streaming form; done when maxd > 0; ev when maxe > 0), row_bits, maxe, maxd, hold_slots or
 * idle_max < 0, C > 2^24: TETRA_E_INVALID, nothing written.  Host or device pointers; with device pointers
 * the call enqueues three kernels on the context stream and returns without waiting (no allocation, no
 * synchronising copy). */
#define TETRA_ASSIGN_HOLD_DEFAULT 720   /* slots, ten multiframes: a stated choice, not a measurement */
#define TETRA_ASSIGN_IDLE_DEFAULT 72    /* bursts of a timeslot, four multiframes: a stated choice likewise */
enum {
    TETRA_AE_ROW = 0, TETRA_AE_BURST, TETRA_AE_BLOCK, TETRA_AE_PDU, TETRA_AE_KIND, TETRA_AE_HEAD, TETRA_AE_CARRIER,
    TETRA_AE_EXT, TETRA_AE_TARGET, TETRA_AE_P_LO, TETRA_AE_P_HI, TETRA_AE_TN, TETRA_AE_FN, TETRA_AE_SSI,
    TETRA_AE_ADDR_TYPE, TETRA_AE_AUX, TETRA_AE_FIELDS = 16
};
enum {
    TETRA_TA_STATE = 0, TETRA_TA_SSI, TETRA_TA_ADDR_TYPE, TETRA_TA_AUX, TETRA_TA_SRC_KEY, TETRA_TA_NALLOC,
    TETRA_TA_IDLE, TETRA_TA_AGE, TETRA_TA_FIELDS = 8
};
typedef struct tetra_etsi_assign_slot {
    int64_t since;                     /* stream bit of the allocation that made the entry active */
    int64_t last;                      /* stream bit of the last allocation or traffic burst */
    int32_t active;
    int32_t ssi, addr_type, aux;       /* of the last allocation */
    int32_t src_key;                   /* key of the carrier that sent it */
    int32_t head;                      /* its 10 head bits */
    int32_t nalloc;                    /* allocations since the entry became active */
    int32_t idle;                      /* decoded control bursts since the last traffic burst */
} tetra_etsi_assign_slot;
typedef struct tetra_etsi_assign_state {   /* per carrier, carried from call to call; all zero = new stream */
    int64_t bit0;                      /* stream bit index of this call's position 0 */
    int32_t expired;                   /* entries freed after hold_slots without a repeat or traffic */
    int32_t released;                  /* entries freed because the slot returned to control signalling */
    tetra_etsi_assign_slot slot[4];    /* timeslots 1..4 */
} tetra_etsi_assign_state;
int tetra_etsi_assign(tetra_ctx *ctx, const int32_t *nsym, size_t C, size_t G, int64_t row_bits, int64_t advance,
                      int32_t hold_slots, int32_t idle_max, int32_t shared_clock, const int32_t *nburst,
                      const int32_t *bursts, const int32_t *nblock, const int32_t *blocks, const int32_t *npdu,
                      const int32_t *pdus, const int32_t *keep /*[C][MAXB] or NULL*/,
                      const int32_t *slots /*[C][MAXB][4] or NULL*/, const int32_t *tq /*[C][MAXB][4] or NULL*/,
                      const int32_t *sdu /*[C][MAXJ][MAXPDU][8]*/, int32_t maxd, const int32_t *ndone /*[C/G]*/,
                      const int32_t *done /*[C/G][maxd][13]*/, const int32_t *row_key /*[C/G] or NULL*/,
                      tetra_etsi_assign_state *state /*[C/G] in/out*/, int32_t maxe, int32_t *nev /*[C/G]*/,
                      int32_t *ev /*[C/G][maxe][16]*/, int32_t *ta /*[C][MAXB][8]*/);

/* The ETSI receiver's AFC mixer on a streaming window: out [C][N] cf32 = iq (cf32 rows ld samples
 * apart) x exp(-j 2 pi f (n0 + n) / fs), n0 = the window's first sample in the capture (frequency_shift's
 * float64 arithmetic, processor.py:85-100, with one continuous phase across windows); mix_c [C] as
 * tetra_demod_compat's (the imaginary part of -1j*2*pi*f). */
int tetra_etsi_mix(tetra_ctx *ctx, const void *iq, size_t C, size_t ld, size_t N, const double *mix_c, double fs,
                   int64_t n0, void *out);

/* Component: decode F type-5 soft blocks of one kind (K = 432/216/120): type1 [F][n1], crc_ok [F]. */
int tetra_etsi_decode_blocks(tetra_ctx *ctx, const int8_t *soft5, size_t F, int kind,
                             const uint32_t *scramb_init, uint8_t *type1, uint8_t *crc_ok);
/* Component: encode F type-1 blocks (CRC, tail, RCPC 2/3, interleave, scramble): type5 [F][K]. */
int tetra_etsi_encode_blocks(tetra_ctx *ctx, const uint8_t *type1, size_t F, int kind,
                             const uint32_t *scramb_init, uint8_t *type5);

/* Synthetic capture generator (device side; bench.py and tests).  Per channel: a continuous
 * downlink of coded bursts (1/2 normal-n, 1/4 normal-p, 1/4 sync), pi/4-DQPSK + RRC(0.35) at fs,
 * random carrier phase, CFO uniform in [-cfo_max, cfo_max] Hz, AWGN at Es/N0 = snr_db (no noise if
 * snr_db >= 200), SC16 quantisation.  Each sync burst's BSCH carries a SYNC PDU of the channel's
 * cell (colour code at type-1 bits 4..9, MCC 31..40, MNC 41..54, the rest random).  Outputs: iq [C][N] cf32, cell_init [C] scrambling inits,
 * and optionally kinds [C][NB] burst kinds, payload [C][NB][2][268] type-1 bits (zero-padded),
 * t0 [C] symbol time of sample 0; NB = tetra_synth_bursts_per_channel(N, fs). */
int tetra_synth_bursts_per_channel(size_t N, double fs);
int tetra_synth_etsi(tetra_ctx *ctx, size_t C, size_t N, double fs, uint64_t seed, float snr_db, float cfo_max,
                     void *iq, uint32_t *cell_init, int32_t *kinds, uint8_t *payload, double *t0);
/* Opt-in slot grid (a context flag, default 0: every output bit for bit as without it).  on != 0:
 * the SYNC PDU of channel ch's burst b carries slot = (tetra_synth_slot0(seed, ch) + b) mod
 * TETRA_TDMA_SLOTS as TN field = slot % 4 (type-1 bits 10..11), FN = slot / 4 % 18 + 1 (12..16), MN =
 * slot / 72 + 1 (17..22) in place of random bits, in tetra_synth_etsi and tetra_synth_wideband. */
int tetra_synth_set_grid(tetra_ctx *ctx, int on);
int tetra_synth_slot0(uint64_t seed, size_t ch);   /* host only: the slot count of channel ch's burst 0 */

/* ---------------------------------------------------------------- wideband channeliser (C3)
 * A fs = 20 MSps capture -> M carriers at fs/M spacing (polyphase filter bank, D = M/4, rocFFT)
 * -> per-carrier RRC(0.35) resampler fs/D -> 72 kHz (up/down) = the ETSI timing stage's input
 * (tetra_etsi_timing).  Replaces tuning the SDR to one carrier per capture (the reference's
 * capture loop, /root/reference/tetraear/ui/modern.py:1886-1887 feeds one 2.4 MSps carrier
 * into SignalProcessor.process); SURVEY.md §8d config C3.  Host pointers h, g. */
typedef struct tetra_wb_plan {
    int32_t M;           /* carriers = FFT length (800) */
    int32_t D;           /* decimation, M / 4 (200): carrier rate fs / D */
    int32_t P;           /* prototype taps per branch, 1..8 (L = M * P) */
    int32_t up, down;    /* carrier resampler fs/D -> 72 kHz (18 / 25) */
    int32_t Lg;          /* resampler taps, a multiple of up */
    double fs;           /* wideband rate */
    const float *h;      /* prototype lowpass [M * P] (unity DC gain) */
    const float *g;      /* resampler RRC at up * fs / D [Lg] */
} tetra_wb_plan;

/* nblk filter-bank output blocks and n72 resampler outputs per carrier for Nw input samples. */
int tetra_wb_lengths(const tetra_wb_plan *plan, size_t Nw, int64_t *nblk, int64_t *n72);
/* x [Nw] cf32 -> y [M][n_keep] cf32 at 72 kHz (first n_keep <= n72 outputs of each carrier; a
 * carrier's row is then n_keep / M2 timing chunks of M2 samples for tetra_etsi_timing). */
int tetra_channelize(tetra_ctx *ctx, const tetra_wb_plan *plan, const void *x, size_t Nw, void *y, size_t n_keep);
/* tetra_channelize that also leaves om [M][ceil(n_keep / up)] float4: per carrier and group of up
 * consecutive outputs, the Oerder-Meyr class partials (sum over o = c mod 4 of |y[up g + o]|^2, o
 * ascending; oracle eo_om_group_partials) for tetra_etsi_timing_chunks (and _om).  D = M / 2 plan (up = 36) only. */
int tetra_channelize_om(tetra_ctx *ctx, const tetra_wb_plan *plan, const void *x, size_t Nw, void *y, size_t n_keep,
                        void *om);
/* The same two entry points for an explicit capture format: iq_fmt TETRA_CF32 (x [Nw] cf32, what
 * the two above pass) or TETRA_SC16 (x [Nw][2] int16, I then Q, each scaled by 1/32768: y and om are
 * those of the cf32 capture x / 32768, bit for bit); any other format is TETRA_E_INVALID.  The
 * default analysis kernels of both designs load SC16 themselves (4 B per sample read); the two-block
 * form (TETRA_WB_ANALYSIS=2) and the unfused fold (M != 800) run behind one conversion pass, and the
 * timing-only TETRA_WB_ANALYSIS_PROBE builds refuse it.  Alignment of x on the device: cf32 as
 * before, 16 bytes (the fused kernels load two samples per lane; not checked); SC16 8 bytes, two
 * samples, which is more than int16 pairs have by nature, so a device pointer that is not is refused
 * with TETRA_E_INVALID before anything is launched (a host array is staged and may sit anywhere).
 * The D = M / 2 kernels address the capture with 32-bit byte offsets, so it must be under 2 GiB:
 * 2^28 samples in cf32, 2^29 in SC16. */
int tetra_channelize_fmt(tetra_ctx *ctx, const tetra_wb_plan *plan, const void *x, int iq_fmt, size_t Nw, void *y,
                         size_t n_keep);
int tetra_channelize_om_fmt(tetra_ctx *ctx, const tetra_wb_plan *plan, const void *x, int iq_fmt, size_t Nw, void *y,
                            size_t n_keep, void *om);
/* Synthetic wideband capture: M carriers of tetra_synth_etsi bursts at fs/D, filter-bank
 * synthesised to fs, plus AWGN at per-carrier Es/N0 = snr_db.  Outputs as tetra_synth_etsi with
 * C = M and N = Nw / D + 1 (carrier k at +k fs / M, i.e. FFT bin k). */
int tetra_synth_wideband(tetra_ctx *ctx, const tetra_wb_plan *plan, size_t Nw, uint64_t seed, float snr_db,
                         float cfo_max, void *x, uint32_t *cell_init, int32_t *kinds, uint8_t *payload, double *t0);

/* ---------------------------------------------------------------- waterfall spectrum (C3)
 * Live spectrum / waterfall rows: frame f of channel c is x[c][f*hop .. f*hop + nfft), Hann
 * window (numpy.hanning), forward FFT, fftshift, power = 20 log10(|X| / nfft + 1e-20) in dBFS --
 * the display of /root/reference/tetraear/ui/modern.py:1928-1941 (one frame x[:2048] per chunk),
 * batched over channels and frames.  iq [C][N] in TETRA_CF32 / TETRA_SC16 / TETRA_CF64; out
 * [C][nframes][nfft] float32.  nfft = 2048 (the reference's fixed size); needs
 * (nframes - 1) * hop + nfft <= N.  Single-pass fused kernel (window + LDS FFT + dB). */
int tetra_waterfall(tetra_ctx *ctx, const void *iq, int iq_fmt, size_t C, size_t N, size_t nfft, size_t hop,
                    size_t nframes, float *out);

/* ---------------------------------------------------------------- FFT resampler
 * SignalProcessor.resample (/root/reference/tetraear/signal/processor.py:35-49 =
 * scipy.signal.resample(x, num)): x [C][Nx] complex (TETRA_CF32 or TETRA_CF64) -> y [C][num] in the
 * same precision; forward rocFFT, spectrum truncation / zero-padding with scipy's Nyquist
 * split/join, inverse rocFFT, scale num/Nx folded in. */
int tetra_resample(tetra_ctx *ctx, const void *x, int fmt, size_t C, size_t Nx, size_t num, void *y);

#ifdef __cplusplus
}
#endif
#endif /* TETRA_HIP_H */
