/*
 * sdr_amd.h -- C ABI of the MI355X-native FM/RDS DSP hot path (libsdr_amd.so, gfx950).
 *
 * Drop-in boundary for TheZxc07/real-time-SDR's per-block DSP (reference paths are relative to
 * the reference repository root). Every entry point is extern "C", takes plain pointers and
 * sizes, returns an int status (SDR_OK = 0) and enqueues work on the caller's HIP stream
 * (`stream` = hipStream_t, NULL = default stream) without synchronising.
 *
 * Data layout (HBM): channel-major batches. A batch of nch independent I/Q streams is
 * `[nch][len]` with a per-channel stride (in elements); per-channel state lives in device memory
 * and is updated in place, exactly like the reference's by-reference state arguments.
 *
 * Numerics: the default ("exact") mode reproduces the reference's rounding points bit for bit:
 * f32 products and sums in tap order without FMA (filter.cpp:111-115), f64 demod denominator
 * and division (demod.cpp:17), f64 atan2/sin/cos rounded to f32 in the PLL (pll.cpp:39-52).
 */
#ifndef SDR_AMD_H
#define SDR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDR_OK 0
#define SDR_E_INVALID (-1)   /* bad argument / shape */
#define SDR_E_HIP (-2)       /* HIP runtime error (see sdr_last_error) */
#define SDR_E_NOMEM (-3)
#define SDR_E_NODEV (-4)     /* no gfx950 device */
#define SDR_E_TIMEOUT (-5)   /* a parity-release wait gave up (a reader held its block > 5 s): the context's
                              * outputs are poisoned from then on; every stage call fails until
                              * sdr_ctx_reset */

#define SDR_MAX_SYMS 256     /* symbols per block, >= n_rds/symbol_Fs + 1 for every mode */
#define SDR_MAX_BITS 256

/* Outputs of a block whose persistent PLL wait timed out (sdr_plls_launch), or of any block after a
 * parity-release wait timed out (SDR_E_TIMEOUT): the output stages write these instead of audio /
 * bits computed from phases that were never produced or from buffers the producer overwrote. */
#define SDR_PCM_POISON ((int16_t)-32768)  /* every L/R sample of the block */
#define SDR_NBITS_POISONED (-2)           /* nbits[ch] of sdr_rds_bits; rds_clean rows are NaN */

/* Context flags */
#define SDR_FLAG_FAST_FRONTEND 0x1  /* int8 MFMA front end, not bit-exact: every fm_demod sample within the derived
                                     * bound tol() of tests/fast_fe_model.py of the f64 definition (I/Q within
                                     * 2^-(F+1) sum|x| + 3 * 2^-24 |y|; tests/test_gpu_fast_frontend.py), and
                                     * within 1e-5 of the reference normwise per block (the north star;
                                     * tests/test_gpu_pipeline.py) */
#define SDR_FLAG_PLL_LIBM 0x2       /* PLL via per-step f64 libm calls (A/B reference) */
#define SDR_FLAG_KEEP_INTERMEDIATES 0x4  /* post stages store every intermediate row (carrier, stereo_dc,
                                          * ipll) for sdr_ctx_buffer; by default the NCO, mixers and
                                          * resamplers are fused and only the rows' history is stored */
#define SDR_FLAG_PHASE_DEMOD 0x8    /* phase discriminator (below): fm_demod is the phase step in radians,
                                     * not its sine; not with SDR_FLAG_FAST_FRONTEND (SDR_E_INVALID) */
#define SDR_FLAG_RDS_QUAD 0x10      /* sdr_rds_post also runs the RDS chain's quadrature branch (below, at
                                     * sdr_ctx_rds_clean_q); mode 0 with rds_on only (SDR_E_INVALID) */
#define SDR_FLAG_IF_ENVELOPE 0x20   /* the exact front ends also store the IF power row "if_env" (below, at
                                     * sdr_meter_rf); not with SDR_FLAG_FAST_FRONTEND (SDR_E_INVALID) */

/* ---- phase discriminator (no reference counterpart; sdr_version stays 3, callers detect it by symbol).
 * fmDemodNoArctan's value is Im(x[n] conj(x[n-1])) / |x[n]|^2 = (|x[n-1]| / |x[n]|) sin(dphi): the sine of
 * the phase step between two IF samples, which stops growing at a deviation of if_Fs / 4 (60, 90, 60,
 * 96 kHz in modes 0-3) and folds beyond it. With SDR_FLAG_PHASE_DEMOD the front end's FIRs are unchanged
 * and every fm_demod sample is the step itself, in radians, in [-RN32(pi), RN32(pi)]. All f32, every
 * product, sum and quotient rounded on its own (no FMA), f32 subnormals kept; (Ip, Qp) is the previous
 * FIR output, the block's first uses the carried one, (0, 0) after create / reset:
 *     re = fl(fl(I Ip) + fl(Q Qp))        im = fl(fl(Q Ip) - fl(I Qp))
 *     a = |re|, b = |im|, mx = max(a, b), mn = min(a, b)
 *     mx == 0            -> +0       (the reference's I = Q = 0 rule, and a zero previous sample)
 *     z = fl(mn / mx)    the correctly rounded quotient;  u = fl(z z)
 *     p = c_K;  p = fl(fl(p u) + c_k) for k = K-1 .. 0;  r = fl(p z)
 *     b > a  -> r = fl(RN32(pi/2) - r);   re < 0 -> r = fl(RN32(pi) - r);   out = copysign(r, im)
 * K = 7: atan(z) ~ z (c_0 + c_1 z^2 + .. + c_7 z^14) on [0, 1], a minimax fit with c_0 = 1 held (so a
 * small step is fl(z) times a factor within an ulp of 1) whose real-arithmetic error is 4.9e-8 rad.
 * Against f64 atan2(im, re) of the same f32 (re, im) the f32 evaluation above is within 2^-20 rad
 * (required, tests/test_demod_model.py); measured over every z = m 2^-24 in all eight octant and sign
 * cases and 10^6 random pairs: 3.39e-7 rad = 0.355 x 2^-20. For small steps the value equals the sine
 * discriminator's, so the audio, the PLL inputs and short(16384 y) keep their scale. */
#define SDR_DEMOD_K 7
#define SDR_DEMOD_C0 0x1p+0f
#define SDR_DEMOD_C1 -0x1.5550f2p-2f
#define SDR_DEMOD_C2 0x1.98d61p-3f
#define SDR_DEMOD_C3 -0x1.1e3d8cp-3f
#define SDR_DEMOD_C4 0x1.912bfep-4f
#define SDR_DEMOD_C5 -0x1.d948p-5f
#define SDR_DEMOD_C6 0x1.797d56p-6f
#define SDR_DEMOD_C7 -0x1.1d6f96p-8f
#define SDR_DEMOD_PI_2 0x1.921fb6p+0f   /* RN32(pi / 2) */
#define SDR_DEMOD_PI 0x1.921fb6p+1f     /* RN32(pi) */
/* host only, no GPU: *n = K + 1, c[0 .. K] filled when c != NULL and max >= K + 1 */
int sdr_demod_coeffs(float *c, int max, int *n);

/* pllblock_args, include/pll.h:10-17 (same field order and types) */
typedef struct sdr_pll_state {
    float feedbackI;
    float feedbackQ;
    float integrator;
    float phaseEst;
    double trigOffset;
    float lastCarrier;   /* the reference keeps it as pllOut[last]; out[0] of the next block */
} sdr_pll_state;

/* Static geometry of a context (mode table of project.cpp:67-108) */
typedef struct sdr_info {
    int nch, mode, rds_on;
    int rf_Fs, rf_decim, if_Fs, audio_upsample, audio_decim, symbol_Fs, rf_taps;
    int block_iq;   /* I/Q pairs per block (rffrontend.cpp:21)          mode 0: 73500 */
    int block_if;   /* fm_demod samples per block                        mode 0: 7350  */
    int n_audio;    /* audio frames per block (mono.cpp:28)             mode 0: 1470  */
    int n_rds;      /* RDS baseband samples per block (rds.cpp:130)      mode 0: 2836  */
    int history;    /* samples of history kept in front of each f32 stream */
} sdr_info;

typedef struct sdr_ctx sdr_ctx;

const char *sdr_last_error(void);
int sdr_version(void);

/* ------------------------------------------------------------------ tap design (host, once)
 * Same formulas, types and rounding as the reference; h must hold num_taps floats. */
int sdr_impulse_response_lpf(float Fs, float Fc, unsigned short num_taps, float *h);            /* filter.cpp:13-29 */
int sdr_impulse_response_lpf_gain(float Fs, float Fc, unsigned short num_taps, int u, float *h); /* filter.cpp:33-50 */
int sdr_impulse_response_bpf(float Fs, const float *Fb, unsigned short num_taps, float *h);     /* filter.cpp:55-71 */
int sdr_impulse_response_apf(float gain, unsigned short num_taps, float *h);                    /* filter.cpp:73-78 */
int sdr_impulse_response_rrc(float Fs, unsigned short num_taps, float *h);                      /* filter.cpp:80-102 */

/* ------------------------------------------------------------------ batched primitives
 * All pointers are device pointers. `state` arrays are [nch][nstate] (nstate >= ntaps-1 for
 * convolveFIR) and hold the previous block's last nstate inputs, zero-initialised by the caller
 * like the reference's std::vector<float>(rf_taps-1). */

/* convolveFIR(y, x, h, state, D): filter.cpp:106-121 (include/filter.h:20). y: [nch][nx/D]. */
int sdr_convolve_fir(float *y, size_t y_stride, const float *x, size_t x_stride, int nch, int nx,
                     const float *h, int ntaps, float *state, int nstate, int D, void *stream);
/* convolveFIR(y, x, h, state, U, D): filter.cpp:123-147 (include/filter.h:24). y: [nch][nx*U/D].
 * Phase restarts at 0 each block; only the last `nstate` (>= 100 for every mode) inputs of the
 * previous block are kept (the reference copies ntaps-1, reading before x). */
int sdr_convolve_fir_resample(float *y, size_t y_stride, const float *x, size_t x_stride, int nch, int nx,
                              const float *h, int ntaps, float *state, int nstate, int U, int D, void *stream);
/* fmDemodNoArctan(I, Q, prevI, prevQ, out): demod.cpp:3-24 (include/demod.h:5). prev: [nch][2]. */
int sdr_fm_demod(float *out, size_t out_stride, const float *I, const float *Q, size_t iq_stride, int nch,
                 int n, float *prev, void *stream);
/* The phase discriminator (SDR_FLAG_PHASE_DEMOD above) on the same arguments: out is the phase step in
 * radians; prev: [nch][2] = the last (I, Q), updated in place. */
int sdr_fm_demod_phase(float *out, size_t out_stride, const float *I, const float *Q, size_t iq_stride, int nch,
                       int n, float *prev, void *stream);
/* fmpll(in, freq, Fs, out, state, ncoScale, phaseAdjust, bw): pll.cpp:4-61 (include/pll.h:20).
 * out: [nch][n+1]; out[ch][0] is set from state[ch].lastCarrier (the previous block's last
 * sample, pll.cpp:18), state[ch].lastCarrier <- out[ch][n]. */
int sdr_fmpll(float *out, size_t out_stride, const float *in, size_t in_stride, int nch, int n, float freq,
              float Fs, sdr_pll_state *state, float ncoScale, float phaseAdjust, float normBandwidth,
              void *stream);
/* cdr(sps, signal): rds_utilities.cpp:4-21 (include/rds_utilities.h:6). offset: [nch] int32.
 * 1 <= sps <= 64, n >= 0; offset i sums the n/sps samples x[k*sps + i]. Each sample is truncated toward
 * zero to int32, where NaN, infinities and values outside int32 count as INT32_MIN; the per-offset sum
 * of the magnitudes is 32 bits and wraps; an offset wins only with a sum > 0 (as int32), the lowest
 * offset wins among equal sums, and the result is 0 when no offset wins. */
int sdr_cdr(int32_t *offset, const float *x, size_t x_stride, int nch, int n, int sps, void *stream);
/* manchester_decode(bits, symbols, block_count, half_symbol, start): rds_utilities.cpp:34-68
 * (include/rds_utilities.h:12). symbols [nch][sym_stride] 0/1 bytes with nsym[ch] valid;
 * state [nch][2] = {half_symbol, start} updated in place; bits [nch][bits_stride] 0/1 bytes,
 * nbits[ch] written. block_count as in the reference (0 selects the alignment search).
 * A call writes at most nsym[ch]/2 + 1 bits per channel (the carried half symbol plus
 * floor(nsym[ch]/2)), so bits_stride >= max nsym/2 + 1. A channel with nsym[ch] <= 0 consumes
 * nothing: nbits[ch] = 0, its {half_symbol, start} stay as they are and no byte of its bits row is
 * written (the reference is undefined there). */
int sdr_manchester_decode(uint8_t *bits, size_t bits_stride, int32_t *nbits, const uint8_t *symbols,
                          size_t sym_stride, const int32_t *nsym, int nch, int block_count, int32_t *state,
                          void *stream);
/* differential_decode(out, bits, last_bit, block_num): rds_utilities.cpp:70-88
 * (include/rds_utilities.h:14). last_bit [nch] int32 updated in place. Where nbits[ch] <= 0, out and
 * last_bit[ch] are left untouched. */
int sdr_differential_decode(uint8_t *out, size_t out_stride, const uint8_t *bits, size_t bits_stride,
                            const int32_t *nbits, int nch, int block_num, int32_t *last_bit, void *stream);

/* ------------------------------------------------------------------ fused pipeline
 * A context owns the taps, every inter-stage buffer and all per-channel state of `nch`
 * channels of one mode on one device: RF_frontend + mono + stereo + rds of the reference
 * (rffrontend.cpp:9-77, mono.cpp:8-50, stereo.cpp:10-115, rds.cpp:11-193) as batched kernels. */
int sdr_ctx_create(sdr_ctx **out, int device, int nch, int mode, int rds_on, int flags);
int sdr_ctx_destroy(sdr_ctx *ctx);
/* all state back to the reference's initial values; clears a release timeout (SDR_E_TIMEOUT) and the
 * last persistent launch's hold on the current block. Call it once the streams that ran the context's
 * stages have drained. */
int sdr_ctx_reset(sdr_ctx *ctx, void *stream);
int sdr_ctx_info(const sdr_ctx *ctx, sdr_info *info);

/* RF_frontend loop body (rffrontend.cpp:58-71): iq [nch][2*block_iq] u8 interleaved I/Q ->
 * the context's fm_demod for this block. Advances the context to the next block. */
int sdr_frontend(sdr_ctx *ctx, const uint8_t *iq, size_t iq_stride, void *stream);
/* The parity-release wait the next sdr_frontend (or sdr_frontend_pre_parts) begins with, enqueued on
 * `stream` now (the producer's wait for its consumers' prepare(), threadsafequeue.h:29-31): that call,
 * on the same stream, then has nothing left to wait for, so a caller can time or order the front-end
 * kernel alone. Optional. */
int sdr_frontend_release_wait(sdr_ctx *ctx, void *stream);
/* Kernel timing of the front end (no reference counterpart; for benchmarks): the next `max_launches`
 * sdr_frontend kernels are timed -- the 101-tap exact and fast (MFMA) front ends by their own
 * workgroups' start and end stamps (s_memrealtime: the earliest start to the latest end, the kernel's
 * span as a rocprofv3 kernel trace sees it), the generic one by HIP events recorded with the launch
 * -- and sdr_frontend_times returns them in ms (synchronising the device). 0 disables; each call
 * re-arms from the first. sdr_frontend_pre_parts launches are not timed. */
int sdr_frontend_timing(sdr_ctx *ctx, int max_launches);
int sdr_frontend_times(sdr_ctx *ctx, double *ms, int max, int *n);
/* The same launches' earliest workgroup start and latest end as raw 100 MHz device ticks (the clock
 * of sdr_plls_timeline), stamping front ends only: where each block's front end sat in the pipeline. */
int sdr_frontend_stamps(sdr_ctx *ctx, unsigned long long *t_start, unsigned long long *t_end, int max, int *n);

/* ---- shared-capture tuner (sdr_version >= 2): many stations from one I/Q stream per front end.
 * Channel ch listens to row src[ch] of a batch of nsrc captures at the mode's rf_Fs and to the station
 * khz[ch] kHz off that capture's centre. With N = rf_Fs / 1000 (2400, 1440, 2400, 1152 for modes 0..3)
 * and n the absolute sample index (block * block_iq + index in the block; the 100 history samples in
 * front of a block are the source row's previous samples, u8 128 before the first block), sample n is
 * multiplied by the rotator T[(khz n) mod N] = (c, s):
 *     y_I = fl(fl(x_I c) + fl(x_Q s)),  y_Q = fl(fl(x_Q c) - fl(x_I s)),  x = (u8 - 128) / 128
 * (four f32 products, two f32 sums, no FMA: (I + jQ) e^(-j 2 pi khz n / N), the station lands at
 * 0 Hz), then the front end's FIR and discriminator as ever. khz = 0 is the identity, bit for bit.
 * The tuned front end always uses these exact numerics: with SDR_FLAG_FAST_FRONTEND it still runs the
 * exact tuned kernel (int8 MFMA operands do not survive the mixer).
 *
 * host only, no GPU: the rotator table of a mode; *n = N, cs = [N][2] (cos, sin)(2 pi i / N), the real
 * values correctly rounded to f32, when cs != NULL and max_pairs >= N */
int sdr_tuner_table(int mode, float *cs, int max_pairs, int *n);
/* src, khz: host arrays [nch]. nsrc rows of capture, 1 <= nsrc <= nch, 0 <= src[ch] < nsrc,
 * -N/2 < khz[ch] <= N/2. Only on a context at block 0 (after create / sdr_ctx_reset); nsrc = 0 removes
 * the tuning. The tuning survives sdr_ctx_reset (it is configuration, like the mode). Synchronises
 * `stream`. A tuned context refuses sdr_frontend and sdr_frontend_pre_parts (SDR_E_INVALID: they would
 * misread the rows); it runs the first block of a persistent launch as sdr_frontend_tuned + sdr_pre +
 * sdr_plls_signal. */
int sdr_tuner_set(sdr_ctx *ctx, int nsrc, const int32_t *src, const int32_t *khz, void *stream);
int sdr_tuner_get(const sdr_ctx *ctx, int *nsrc);          /* 0: not tuned */
/* host only, no GPU: SDR_OK when sdr_tuner_set takes this tuning on a context of nch channels in `mode` */
int sdr_tuner_check(int mode, int nch, int nsrc, const int32_t *src, const int32_t *khz);
/* RF_frontend loop body for a tuned context: iq [nsrc][2*block_iq]. Same parity-release wait, timing
 * hooks (sdr_frontend_timing armed after sdr_tuner_set) and block advance as sdr_frontend. */
int sdr_frontend_tuned(sdr_ctx *ctx, const uint8_t *iq, size_t iq_stride, void *stream);

/* ---- band scan (sdr_version >= 3): where the stations sit in the capture rows the tuner shares.
 * A batched power spectrum in the manner of the reference's estimatePSD (src/fourier.cpp:
 * non-overlapping segments, Hann window, |X|^2 per bin, average over segments) whose bins are the
 * tuner's 1 kHz steps: N = rf_Fs / 1000 as above, and a station that sdr_tuner_set reaches with
 * khz = +f is a peak at bin f mod N (bin k is khz = k for k <= N/2 and k - N above it).
 * A block of a row is cut into S_b = block_iq / N (30, 36, 33, 33 for modes 0..3) consecutive
 * segments of N samples from the block's first sample on; the rest of the block is not used,
 * segments never straddle blocks and there is no history. Per segment, in f32:
 *     x = (u8 - 128) / 128,  w[j] = RN32(0.5 - 0.5 cos(2 pi j / N)) (evaluated in f64),
 *     X[k] = sum_n x[n] w[n] e^(-j 2 pi k n / N),  p[k] = re^2 + im^2
 * (a mixed-radix DFT, N = 48 x 50, 36 x 40, 32 x 36, whose every twiddle is an entry of
 * sdr_tuner_table), and A[row][k] += sum over the block's segments of p[k] in a fixed order: a row's
 * result is bit-identical from run to run and whatever other rows share the batch.
 * psd[row][k] = A / S, S the segments accumulated since the last reset; no other normalisation, no dB.
 *
 * host only, no GPU: */
typedef struct sdr_scan sdr_scan;
int sdr_scan_geometry(int mode, int *n_bins, int *segments_per_block, int *block_iq);   /* any may be NULL */
/* the f32 Hann table: *n = N, w filled when w != NULL and max >= N */
int sdr_scan_window(int mode, float *w, int max, int *n);
typedef struct sdr_scan_opts {
    int half_width_khz, step_khz, first_khz, sep_khz, guard_khz;
    float thr_db;
} sdr_scan_opts;
void sdr_scan_opts_default(sdr_scan_opts *o);   /* 100, 100, 0, 150, 100, 10.0f */
/* The stations of one spectrum row, deterministic, all arithmetic in double on the f32 input:
 *   channel power  C[k] = sum_{d = -W..W} psd[(k + d) mod N] (added in ascending d), W = half_width_khz
 *   floor          F = the lower median of C over all N bins (element (N - 1) / 2 of the sorted values)
 *   candidates     every khz with -N/2 + guard <= khz <= N/2 - guard and (khz - first_khz) mod step == 0
 *                  (with guard = 0 both -N/2 and N/2 are candidates; they name the same bin)
 *   a candidate is a station when C > 0, C >= F 10^(thr_db / 10), and no other candidate within
 *   |delta khz| <= sep_khz has a larger C, or an equal C at a lower khz.
 * Output in descending C, ties in ascending khz; db = 10 log10(C / F) (HUGE_VALF when F = 0). *n is
 * the number found even when larger than max; at most max are written. SDR_E_INVALID unless
 * 0 <= W < N/2, step >= 1, sep >= 0, 0 <= guard <= N/2 and thr_db is finite. */
int sdr_scan_pick(int mode, const float *psd_row /*[N]*/, const sdr_scan_opts *o, int32_t *khz, float *db, int max,
                  int *n);
/* device: the scanner is its own handle (no channels, no sdr_ctx); it may run on its own stream beside
 * a running pipeline, on the same device buffer sdr_frontend_tuned reads. SDR_E_INVALID for a bad
 * mode, nsrc < 1, a short or odd stride, or NULL pointers (nothing is enqueued then). */
int sdr_scan_create(sdr_scan **out, int device, int mode, int nsrc);
int sdr_scan_destroy(sdr_scan *s);
int sdr_scan_reset(sdr_scan *s, void *stream);                        /* accumulator and S back to 0 */
/* iq [nsrc][2*block_iq], exactly sdr_frontend_tuned's input (same stride and alignment rule; rows
 * whose first byte is 16-byte aligned load fastest); enqueues, no sync */
int sdr_scan_block(sdr_scan *s, const uint8_t *iq, size_t iq_stride, void *stream);
/* psd: host [nsrc][N]; *segments = S per row (psd is all zero while S = 0); synchronises `stream` */
int sdr_scan_psd(sdr_scan *s, float *psd, long long *segments, void *stream);

/* ---- wideband splitter (no reference counterpart; sdr_version stays 3, callers detect it by symbol):
 * one wide signed 8-bit I/Q capture at W * rf_Fs (W = 4, 8 or 10; a HackRF's 19.2 MS/s is W = 8 in mode 0)
 * into the R = 2 W - 1 half-overlapping u8 capture rows at rf_Fs that sdr_frontend_tuned and
 * sdr_scan_block read. With N = rf_Fs / 1000, row r has k = r - (W - 1) and its centre k N / 2 kHz off the
 * wide capture's centre: a station at F = k N / 2 + d kHz of the wide capture is the station khz = +d of
 * row r, and every station lies within N / 4 of some row's centre. All integer, so every correct
 * implementation gives the same bytes.
 *   input    [nwide][2 W block_iq] int8, I then Q; x[n] = sample n of a stream counted from the last
 *            reset, x[n] = 0 for n < 0 (the handle carries the last T - 1 samples from block to block)
 *   taps     T = 16 W, int16 g[r][m] = (g_re, g_im), in f64 and rounded to nearest (rint):
 *                u = m - (T - 1) / 2,  sinc(x) = sin(pi x) / (pi x)
 *                h = sinc(u / W) (0.42 - 0.5 cos(2 pi (m + 1/2) / T) + 0.08 cos(4 pi (m + 1/2) / T))
 *                theta = pi ((k (2 m - T + 1)) mod 4 W) / (2 W)      (the integer reduced first, to [0, 4 W))
 *                g_re = rint(8191 h cos theta),  g_im = rint(8191 h sin theta)
 *            (flat within 0.01 dB to N / 4 + 128 kHz of the row's centre, aliases into that region at
 *            least 71 dB down, max |g| = 8156)
 *   output   sample t (absolute: block * block_iq + index) of row r, in int32 (|acc| < 2.4e8):
 *                acc_re = sum_m g_re[m] x_I[W t - m] - g_im[m] x_Q[W t - m]
 *                acc_im = sum_m g_re[m] x_Q[W t - m] + g_im[m] x_I[W t - m]
 *                if k t is odd: acc = -acc            (the row lands at 0 Hz, not at rf_Fs / 2)
 *                v = 128 + ((acc + (1 << (shift - 1))) >> shift)    (arithmetic shift)
 *                out = clamp(v, 0, 255); each component with v < 0 or v > 255 adds 1 to clips[stream][r]
 *            shift in 1..24, default 14, 15, 16 for W = 4, 8, 10 (DC gain 2.0, 2.0, 1.25).
 *   rows     output row w R + r is stream w, row r: u8 I/Q, 2 block_iq bytes, row_stride apart.
 *
 * host only, no GPU (any output pointer may be NULL): rows = R, taps = T, wide_iq = W block_iq,
 * half_khz = N / 2 (the spacing of the row centres), shift_default */
typedef struct sdr_split sdr_split;
int sdr_split_geometry(int mode, int W, int *rows, int *taps, int *wide_iq, int *half_khz, int *shift_default);
/* the tap table: *n = R T, g = [R][T][2] filled when g != NULL and max_pairs >= R T */
int sdr_split_taps(int W, int16_t *g, int max_pairs, int *n);
/* device: the splitter is its own handle (no sdr_ctx); it may run on any stream beside a running
 * pipeline. shift <= 0 takes the default. SDR_E_INVALID, with nothing enqueued, for a bad mode, W, nwide
 * (1..4096) or shift, NULL pointers, wide_stride < 2 W block_iq or no multiple of 4, wide not 4-byte
 * aligned, or a rows / row_stride that sdr_frontend_tuned would refuse (row_stride >= 2 block_iq, both
 * even; 4-byte aligned rows are stored in whole dwords). */
int sdr_split_create(sdr_split **out, int device, int mode, int W, int nwide, int shift);
/* host only, no GPU: SDR_OK when sdr_split_create takes these arguments */
int sdr_split_check(int mode, int W, int nwide, int shift);
int sdr_split_destroy(sdr_split *s);
int sdr_split_reset(sdr_split *s, void *stream);     /* history and clip counters back to 0 */
/* one block of every stream: one launch on `stream`, no sync */
int sdr_split_block(sdr_split *s, const int8_t *wide, size_t wide_stride, uint8_t *rows, size_t row_stride,
                    void *stream);
/* clips: host [nwide * R], accumulated since the last reset; synchronises `stream` */
int sdr_split_clips(sdr_split *s, long long *clips, void *stream);

/* ---- 16-bit wideband splitter (no reference counterpart; sdr_version stays 3, callers detect it by symbol):
 * the splitter above for the sc16 stream of a USRP, bladeRF, LimeSDR, Pluto or SDRplay, with a shift per stream
 * and row and a peak reading per row, so that a row that holds only a weak station gets its own gain. W, R, T,
 * the taps (exactly sdr_split_taps(W): no new table), the rows, the history and the sign flip are as above.
 * All integer, so every correct implementation gives the same bytes, clip counts and peaks.
 *   input    [nwide][2 W block_iq] little-endian int16, I then Q (4 W block_iq bytes per stream and block);
 *            zeros before the first block and after a reset
 *   sums     acc_re, acc_im: the formulas above on the 16-bit samples, in 64-bit integers, negated when k t is
 *            odd. With the shipped taps max_col sum |e| is 75012, 148820, 185844 for W = 4, 8, 10, so |acc| is
 *            at most 2.46e9, 4.88e9, 6.09e9: under 2^33 and over 2^31 for every W
 *   output   v = 128 + ((acc + (1 << (s - 1))) >> s)          (arithmetic shift on int64)
 *            s = shift[stream][r] in 1..33, a shift per stream and row; default 22, 23, 24 for W = 4, 8, 10
 *            (the s8 defaults + 8: the same gain relative to full scale)
 *            out = clamp(v, 0, 255); each component with v < 0 or v > 255 adds 1 to clips[stream][r]
 *   peaks    peaks[stream][r] = max of max(|acc_re|, |acc_im|) over every output sample of the row since the
 *            last reset or clearing read; it does not depend on the shifts
 *   gain     sdr_split16_shift_for(peak, target, W), target in 1..127 (90 is the usual one): with
 *            rnd(p, s) = (p + (1 << (s - 1))) >> s, the smallest s in 1..33 with rnd(peak, s) <= target; W's
 *            default for peak == 0. A block whose peaks chose the shifts clips nothing when split with them,
 *            and every row given s > 1 then has an output excursion max |out - 128| >= target / 2 (floor).
 *   An s8 capture widened as 256 x and split with shift s + 8 on every row gives the rows and clips of sdr_split
 *   at shift s ((256 a + 2^(s+7)) >> (s + 8) == (a + 2^(s-1)) >> s); so does the same capture sign-extended, at
 *   shift s (s in 1..24).
 *
 * Geometry: sdr_split_geometry (a wide block is 2 wide_iq int16 values). shift <= 0 takes the default.
 * SDR_E_INVALID, with nothing enqueued and nothing changed, for a bad mode, W, nwide (1..4096) or shift, a shifts
 * table with a value outside 1..33, NULL pointers, wide_stride (in bytes) < 4 W block_iq or no multiple of 4, wide
 * not 4-byte aligned, or a rows / row_stride that sdr_split_block would refuse. */
typedef struct sdr_split16 sdr_split16;
int sdr_split16_create(sdr_split16 **out, int device, int mode, int W, int nwide, int shift);
/* host only, no GPU: SDR_OK when sdr_split16_create takes these arguments */
int sdr_split16_check(int mode, int W, int nwide, int shift);
int sdr_split16_destroy(sdr_split16 *s);
/* history, clip counters and peaks back to 0; the shifts stay as they are */
int sdr_split16_reset(sdr_split16 *s, void *stream);
/* shifts: host [nwide * R], all judged first. Ordered on `stream` like a block call: it holds for the block
 * calls enqueued after it, no sync (the table lives in device memory; the caller's array may go at once) */
int sdr_split16_set_shifts(sdr_split16 *s, const int *shifts, void *stream);
/* one block of every stream: one launch on `stream`, no sync */
int sdr_split16_block(sdr_split16 *s, const int16_t *wide, size_t wide_stride, uint8_t *rows, size_t row_stride,
                      void *stream);
/* clips, peaks: host [nwide * R], since the last reset (peaks: or clearing read, clear != 0); synchronise `stream` */
int sdr_split16_clips(sdr_split16 *s, long long *clips, void *stream);
int sdr_split16_peaks(sdr_split16 *s, long long *peaks, int clear, void *stream);
/* host only, no GPU: the gain rule above; SDR_E_INVALID (negative) for a bad target, W or a negative peak */
int sdr_split16_shift_for(long long peak, int target, int W);

/* ---- reception meter (no reference counterpart; sdr_version stays 3, callers detect it by symbol):
 * per channel and block, what a receiver's stereo lamp and tuning indicator show, reduced on the GPU
 * from rows the pipeline already keeps. n = block_if, x = the block's fm_demod row, x[-100..-1] the
 * previous block's tail (zeros before block 0):
 *   fm_sum, fm_sq, fm_peak   sum x, sum x^2, max |x| (NaN ignored)
 *   pilot_sq                 sum pilot^2 over the 19 kHz pilot row (sdr_stereo_pre)
 *   noise_sq                 sum y^2, y[j] = sum_{k=0..100} h_n[k] x[5j - k], j < n/5, with
 *                            h_n = sdr_impulse_response_bpf(if_Fs, {75e3, 84e3}, 101): the discriminator's
 *                            noise in the gap between the 67 and 92 kHz SCA sub-carriers, every fifth point
 *   rds_sq                   sum rds_band^2 over the 57 kHz RDS band row (sdr_rds_pre)
 *   eye_abs, eye_sq, eye_n   s_k = |rds_clean[off + k symbol_Fs]| for every index below n_rds, with
 *                            off = cdr(symbol_Fs, rds_clean) run by the meter on every block (whatever
 *                            sdr_rds_bits does): sum s_k, sum s_k^2 and their count
 *   l_peak, r_peak, l_sq, r_sq   max |s| and sum s^2 of the int16 L and R samples, exact integers
 * Numerics: every f32 product and sum is rounded on its own (no FMA), a square is fl(v v), the noise
 * FIR adds its products in ascending k from +0 (convolveFIR, filter.cpp:106-121). A float sum over a
 * row of length m: partial p (0 <= p < 256) adds the elements i = p (mod 256) in ascending i from +0;
 * then P[p] = fl(P[p] + P[p + w]) for p < w, w = 128, 64, .., 1; the result is P[0]. The eye sums use
 * 64 partials and six levels. A row is therefore bit-identical from run to run and whatever the batch.
 * Units: the discriminator is fmDemodNoArctan, whose output is about the sine of the phase step, not
 * the step: the readings are discriminator units and ratios of them, NOT deviation in kHz (the
 * 7.5 kHz pilot of the synthetic multiplex reads about 1.46 kHz under the small-signal conversion
 * if_Fs / 2 pi). */
typedef struct sdr_meter_row {   /* 64 bytes */
    float fm_sum, fm_sq, fm_peak, pilot_sq, noise_sq, rds_sq, eye_abs, eye_sq;
    int32_t eye_n, flags;        /* flags: SDR_METER_ROW_* */
    int32_t l_peak, r_peak;
    uint64_t l_sq, r_sq;
} sdr_meter_row;
/* row flags: that part of the row holds a reading, written by its call on that call's current block;
 * set by the first such call after create / sdr_meter_reset */
#define SDR_METER_ROW_AUDIO 0x1  /* sdr_meter_audio: fm_*, pilot_sq, noise_sq, l_*, r_* */
#define SDR_METER_ROW_RDS 0x2    /* sdr_meter_rds: rds_sq, eye_* */
typedef struct sdr_meter sdr_meter;
/* host only, no GPU: the noise band-pass of a mode; *n = 101, h filled when h != NULL and max >= 101 */
int sdr_meter_taps(int mode, float *h, int max, int *n);
typedef struct sdr_meter_opts {
    float pilot_nr_min, rds_nr_min, offtune_min;
    int silence_peak;
} sdr_meter_opts;
void sdr_meter_opts_default(sdr_meter_opts *o);   /* 1.0f, 4.0f, 0.25f, 64 */
#define SDR_METER_STEREO 0x1     /* pilot_nr >= pilot_nr_min */
#define SDR_METER_RDS 0x2        /* rds_nr >= rds_nr_min */
#define SDR_METER_OFFTUNE 0x4    /* |offset| >= offtune_min */
#define SDR_METER_DEAD_AIR 0x8   /* the audio part is written and l_peak, r_peak <= silence_peak */
typedef struct sdr_meter_state {
    double offset, level_db, pilot_nr, rds_nr, eye_db;
    int flags;                   /* SDR_METER_STEREO | ... */
} sdr_meter_state;
/* One row's readings, in double on the row's values (n = block_if of the mode):
 *   offset = fm_sum / n,  level_db = 10 log10(fm_sq / n)
 *   pilot_nr = (pilot_sq / n) / (noise_sq / (n / 5)),  rds_nr likewise from rds_sq
 *   eye_db = 10 log10(m1^2 / (m2 - m1^2)),  m1 = eye_abs / eye_n,  m2 = eye_sq / eye_n
 * A ratio with a zero numerator (or eye_n = 0) is 0, one with a zero denominator under a positive
 * numerator is +infinity; the dB of 0 is -infinity. */
int sdr_meter_status(int mode, const sdr_meter_row *row, const sdr_meter_opts *o, sdr_meter_state *out);
/* One row's discriminator readings as FM deviation in kHz, in double (n = block_if, k = if_Fs / (2 pi 1000)):
 *   peak_khz = k fm_peak,  rms_khz = k sqrt(fm_sq / n),  offset_khz = k fm_sum / n
 * Meaningful only for rows of a context with SDR_FLAG_PHASE_DEMOD, whose fm_demod is the phase step in
 * radians; on a default context's rows the same formula is the small-signal conversion the note above
 * warns about. Host only, no GPU; any output pointer may be NULL. */
int sdr_meter_deviation(int mode, const sdr_meter_row *row, double *peak_khz, double *rms_khz, double *offset_khz);
/* device: the meter is its own handle, like the scanner; it owns the taps and rows[nch] (all zero after
 * create and sdr_meter_reset). Both calls enqueue one kernel on `stream` and write their fields of every
 * channel's row for `ctx`'s current block; they may use two contexts (an audio and an RDS one joined by
 * sdr_push_fm_demod) and two streams and still fill one row.
 *   sdr_meter_audio  fm_*, pilot_sq, noise_sq and the audio fields; needs sdr_stereo_pre (or sdr_pre)
 *                    of the block. lr is the row sdr_stereo / sdr_stereo_post wrote for it, ordered by
 *                    the caller; NULL leaves the audio fields 0.
 *   sdr_meter_rds    rds_sq and the eye fields; needs sdr_rds_pre and sdr_rds_post (or sdr_rds_dsp) of
 *                    the block, on this stream or ordered before it (rds_clean is not a parity buffer:
 *                    the rule of sdr_rds_bits).
 * The meter is a reader in the parity-release protocol (fm, pilot and rds_band belong to the block's
 * parity): the producers of the block two later wait for it as for sdr_stereo_post; a context no meter
 * call ran on waits for nothing new. SDR_E_INVALID, nothing enqueued: NULL handles, a context of
 * another nch, mode or device, a short lr_stride, a stage that has not run for the current block,
 * rds_on = 0 in sdr_meter_rds. SDR_E_TIMEOUT as every stage call. */
int sdr_meter_create(sdr_meter **out, int device, int nch, int mode);
int sdr_meter_destroy(sdr_meter *m);
int sdr_meter_reset(sdr_meter *m, void *stream);
int sdr_meter_audio(sdr_meter *m, sdr_ctx *ctx, const int16_t *lr, size_t lr_stride, void *stream);
int sdr_meter_rds(sdr_meter *m, sdr_ctx *ctx, void *stream);
/* host_rows [nch]; synchronises `stream` */
int sdr_meter_read(sdr_meter *m, sdr_meter_row *host_rows, void *stream);
int sdr_meter_rows(sdr_meter *m, const sdr_meter_row **dev);   /* the device rows [nch] */

/* ---- reception meter, RF readings (no reference counterpart; sdr_version stays 3, callers detect it by
 * symbol): the station's level at the antenna and the steadiness of its envelope, which no row behind
 * the discriminator holds (the discriminator divides the level out).
 * The row. A context created with SDR_FLAG_IF_ENVELOPE keeps, per block and channel, the IF power
 *     if_env[c] = fl(fl(I I) + fl(Q Q)),  c = 0 .. block_if - 1
 * of the decimating FIR's f32 outputs (I, Q) the discriminator reads (rffrontend.cpp:67-68; tuned: the
 * same FIR behind the mixer): one f32 square each and one f32 sum, each rounded on its own, no FMA.
 * sdr_frontend, sdr_frontend_tuned and sdr_frontend_pre_parts write it (every c exactly once) next to
 * fm_demod, with or without SDR_FLAG_PHASE_DEMOD; fm_demod and every other result stay bit for bit what
 * they are without the flag. It is a parity buffer [2][nch][block_if] like fm_demod, "if_env" of
 * sdr_ctx_buffer (stride as "fm"); SDR_E_INVALID there on a context without the flag, before the first
 * front end (also after sdr_ctx_reset), and while the current block is one sdr_push_fm_demod brought (it
 * brings no I/Q). Without the flag nothing is allocated and the front ends run as they always did.
 * The reading, over e = the block's if_env row, n = block_if:
 *   env_sum, env_sq    sum e[i], sum fl(e[i] e[i]), by the meter's summation rule above (256 partials,
 *                      partial p adding i = p (mod 256) in ascending i from +0, then eight pairing levels)
 *   env_max, env_min   max e from 0, min e from +infinity; NaN ignored, as for fm_peak (u8 samples and
 *                      finite taps cannot make one)
 *   n                  block_if of the block read; flags: SDR_METER_ROW_RF once written; reserved: 0 */
typedef struct sdr_meter_rf_row {   /* 32 bytes */
    float env_sum, env_sq, env_min, env_max;
    int32_t n, flags;
    int32_t reserved[2];
} sdr_meter_rf_row;
#define SDR_METER_ROW_RF 0x4     /* sdr_meter_rf: the whole sdr_meter_rf_row */
/* device: a second array rf_rows[nch] of the meter handle, all zero after create and sdr_meter_reset.
 * sdr_meter_rf enqueues one kernel on `stream` (one workgroup of 256 threads per channel, one pass over
 * the row) that writes every channel's row for `ctx`'s current block with plain stores; it shares no word
 * with sdr_meter_audio / sdr_meter_rds, so it may run next to them on other contexts and streams. It is
 * a reader in the parity-release protocol with a slot of its own: the front end of the block two later
 * waits for it; a context no sdr_meter_rf ran on waits for nothing new. `stream` is the front end's, or
 * one the caller ordered behind it. SDR_E_INVALID, nothing enqueued: NULL handles, a context of another
 * nch, mode or device, a context without SDR_FLAG_IF_ENVELOPE, no front end yet, a current block that
 * sdr_push_fm_demod brought. SDR_E_TIMEOUT as every stage call. */
int sdr_meter_rf(sdr_meter *m, sdr_ctx *ctx, void *stream);
/* host_rows [nch]; synchronises `stream` */
int sdr_meter_rf_read(sdr_meter *m, sdr_meter_rf_row *host_rows, void *stream);
int sdr_meter_rf_rows(sdr_meter *m, const sdr_meter_rf_row **dev);   /* the device rows [nch] */
typedef struct sdr_meter_rf_opts { float ripple_max; } sdr_meter_rf_opts;
void sdr_meter_rf_opts_default(sdr_meter_rf_opts *o);   /* 21.0f / 121.0f */
#define SDR_METER_RF_WEAK 0x1    /* the row is written and m1 == 0 or ripple > ripple_max */
typedef struct sdr_meter_rf_state {
    double level_dbfs, ripple, cnr_db, fade_db, crest_db;
    int flags;                   /* SDR_METER_RF_WEAK */
} sdr_meter_rf_state;
/* One row's readings, host only, in double on the row's values, m1 = env_sum / n, m2 = env_sq / n (both 0
 * for n <= 0: an unwritten row):
 *   level_dbfs = 10 log10(m1): 0 dBFS is a carrier of amplitude 1.0 in the front end's (u8 - 128) / 128
 *                scale, in the passband
 *   ripple     = (m2 - m1^2) / m1^2, the normalised variance of the IF power: 0 for a constant envelope,
 *                1 for Gaussian noise alone; 0 when m1 == 0
 *   cnr_db     the second/fourth-moment estimate for a constant-modulus carrier S in complex Gaussian noise
 *                N (M2 = S + N, M4 = S^2 + 4 S N + 2 N^2): S = sqrt(max(2 m1^2 - m2, 0)), N = m1 - S,
 *                cnr_db = 10 log10(S / N); -infinity when S = 0, +infinity when N <= 0 and S > 0
 *   fade_db    = 10 log10(env_min / m1), crest_db = 10 log10(env_max / m1): the block's deepest null and
 *                highest peak; both 0 when m1 == 0
 * The dB of 0 is -infinity. The model gives ripple = (2 r + 1) / (r + 1)^2 at a C/N of r, so the default
 * ripple_max = 21/121 is r = 10, the textbook FM threshold: derived, not measured.
 * n makes rows summable: adding env_sum, env_sq and n of several blocks in double and taking the minimum
 * of env_min and the maximum of env_max gives a run-long row that this function reads as well (the
 * receiver engine's PREFIX.rfstatus).
 * Limits. The level is relative to the full scale of the row the front end read; in a wideband run that
 * is the splitter's output row, and its shift (PREFIX.wide) converts it. cnr_db is a lower bound: whatever
 * puts AM on the carrier -- multipath, a co-channel, the 100 kHz channel filter acting on a fully deviated
 * signal -- reads as noise. Measured on the model with the front end's own taps (lpf(2.4e6, 1e5, 101), mode
 * 0, a carrier of amplitude 0.3 as u8 input, four blocks = 29400 IF samples per figure, tests/rf_model.py):
 *   - an unmodulated carrier in noise reads within 0.1 dB of its true in-channel C/N from 6 to 22 dB, and
 *     0.35 to 0.8 dB high from 4 dB down to 0 dB; noise-free it reads 68.6 dB (the u8 rounding);
 *   - clean, noise-free FM at 75 kHz deviation on a centred carrier caps the estimate at 27.8 dB (1 kHz tone)
 *     and 22.0 dB (15 kHz tone); with the carrier 20 kHz off centre, where the deviation reaches the filter's
 *     edge, at 15.3 dB;
 *   - at 22 dB of true C/N, 75 kHz deviation on a centred carrier reads 1.1 dB (1 kHz tone) and 3.1 dB (15 kHz
 *     tone) low, 20 kHz off centre 7.6 dB low.
 * SDR_E_INVALID: NULL arguments, a mode outside 0..3. */
int sdr_meter_rf_status(int mode, const sdr_meter_rf_row *row, const sdr_meter_rf_opts *o, sdr_meter_rf_state *out);

/* ---- audio finishing (no reference counterpart; sdr_version stays 3, callers detect it by symbol):
 * de-emphasis, a stereo blend driven by the meter's pilot reading, and a gain, over the int16 rows
 * sdr_stereo / sdr_stereo_post (width 2, L/R interleaved) or sdr_mono (width 1) wrote. The rows in and
 * out are the caller's, so the stage is outside the parity-release protocol. N = n_audio,
 * Fs_a = if_Fs * audio_upsample / audio_decim (48000, 40000, 44100, 44100 Hz in modes 0-3).
 * Coefficients, on the host in double: a = RN32(exp(-1e6 / (tau_us Fs_a))), b = RN32(1 - (double)a);
 * tau_us = 0: a = 0, b = 1, no de-emphasis.
 * State per channel (sdr_audio_state): y[2], the current blend g0 and gain v0, the targets g1 and v1;
 * after create and sdr_audio_reset y = 0 and g0 = g1 = v0 = v1 = 1.
 * One call, frames n = 0 .. N-1, every f32 product and sum rounded on its own (no FMA), f32 subnormals
 * kept: rN = fl(1.0f / (float)N), dg = fl(g1 - g0), dv = fl(v1 - v0), then
 *   t = fl((float)(n + 1) rN),  g = fl(g0 + fl(dg t)),  v = fl(v0 + fl(dv t))
 *   l = (float)L[n], r = (float)R[n],  m = 0.5f (l + r),  s = 0.5f (l - r)          (both exact)
 *   p = fl(g s),  xl = fl(m + p),  xr = fl(m - p)
 *   yl = fl(fl(a yl) + fl(b xl)), yr likewise
 *   out = (int16) clamp(rintf(fl(v y)), -32767, 32767)     (rintf: to nearest even; -32768 is never
 *                                                           made from audio, it stays SDR_PCM_POISON)
 * and afterwards g0 := g1, v0 := v1: a change of blend or gain is a linear ramp over one block, free of
 * clicks. Width 1: x = (float)s[n], one y, no blend. A row whose width N input samples all equal
 * SDR_PCM_POISON is poisoned: its output is all SDR_PCM_POISON and the channel's y becomes 0; the ramps
 * still advance. A channel's bytes do not depend on the batch it is in.
 * Fidelity: the one-pole is the impulse-invariant filter, not the analogue RC network
 * 1 / sqrt(1 + (2 pi f tau)^2): it attenuates LESS than the network by 0.01 dB at 1 kHz, 0.15-0.22 dB
 * at 5 kHz, 0.6-0.9 dB at 10 kHz and 1.4-2.1 dB at 15 kHz (tau 50 and 75 us, the four audio rates). */
typedef struct sdr_audio sdr_audio;
typedef struct sdr_audio_opts {
    float tau_us, blend_lo, blend_hi;
} sdr_audio_opts;
void sdr_audio_opts_default(sdr_audio_opts *o);   /* 75, 0.5, 2.0 */
/* host only, no GPU: the one-pole's coefficients of a mode */
int sdr_audio_coeffs(int mode, float tau_us, float *a, float *b);
/* host only, no GPU: SDR_OK when sdr_audio_create takes the record in `mode` (tau_us, blend_hi > blend_lo) */
int sdr_audio_opts_check(int mode, const sdr_audio_opts *opts);
typedef struct sdr_audio_state {   /* 24 bytes */
    float y[2], blend, gain, blend_target, gain_target;
} sdr_audio_state;
/* The stage is its own handle, like the meter. Every call enqueues on `stream` and returns;
 * sdr_audio_read_state synchronises.
 *   sdr_audio_set_control       blend and gain: host arrays [nch] of new targets, either may be NULL
 *                               (that target stays); they take effect as a ramp over the next block
 *   sdr_audio_blend_from_meter  the blend target of every channel from the meter's device row, in f32,
 *                               n = block_if, q = n / 5 (integer): a row without SDR_METER_ROW_AUDIO leaves
 *                               the target as it is; else P = fl(pilot_sq (float)q), Z = fl(noise_sq (float)n);
 *                               !(P > 0): 0; Z == 0: 1; else min(max(fl(fl(fl(P / Z) - blend_lo) /
 *                               fl(blend_hi - blend_lo)), 0), 1), NaN giving 0 (P / Z is the meter's
 *                               pilot_nr; the division is the correctly rounded one). It must be ordered
 *                               after the sdr_meter_audio whose row it reads: the same stream, or the caller.
 *   sdr_audio_finish            one block: in [nch][>= width N] to out [nch][>= width N], strides in
 *                               int16; out == in with equal strides is allowed, any other overlap is
 *                               the caller's error
 * SDR_E_INVALID, nothing enqueued: NULL handles or pointers, a bad mode, nch < 1, width not 1 or 2, tau_us
 * negative, not finite or above 1000, blend_hi <= blend_lo, a blend outside [0, 1], a gain negative or not
 * finite, a stride below width N or odd, a base not 4-byte aligned, a meter of another nch, mode or
 * device. */
int sdr_audio_create(sdr_audio **out, int device, int nch, int mode, int width, const sdr_audio_opts *o);
int sdr_audio_destroy(sdr_audio *a);
int sdr_audio_reset(sdr_audio *a, void *stream);
int sdr_audio_set_control(sdr_audio *a, const float *blend, const float *gain, void *stream);
int sdr_audio_blend_from_meter(sdr_audio *a, sdr_meter *m, void *stream);
int sdr_audio_finish(sdr_audio *a, const int16_t *in, size_t in_stride, int16_t *out, size_t out_stride, void *stream);
/* host [nch]; synchronises `stream` */
int sdr_audio_read_state(sdr_audio *a, sdr_audio_state *host, void *stream);

/* ---- RDS group decoder (no reference counterpart; sdr_version stays 3, callers detect it by symbol):
 * block synchronisation with a flywheel, +-1 bit slip recovery and burst-error correction over the bits
 * sdr_rds_bits wrote, per channel on the GPU, and a host text layer over the 16-byte group records. All
 * integer; tests/rds_model.py defines every bit, DESIGN.md section 4g explains the rules.
 * Coding (IEC 62106): g(x) = 0x5B9; the syndrome of a 26-bit word (first bit received = bit 25) is its
 * remainder modulo g; offset words A, B, C, C', D = 0x0FC, 0x198, 0x168, 0x350, 0x1B4 of block indices
 * 0, 1, 2, 2, 3; a word matches offset o when its syndrome equals the offset word.
 * Correction table: every error pattern e whose set bits span at most max_burst of the 26 positions,
 * tab[syndrome(e)] = e (51 entries at max_burst 2, 367 at 5, all syndromes distinct), 0 elsewhere.
 * Per channel and bit i (counted from the last reset), after shifting it in:
 *   not synchronised, from the 26th bit on: a latest-26 word that matches an offset of block index idx is a
 *     hit. With a pending hit (p, q), d = i - p, d % 26 == 0, 1 <= d / 26 <= 4 and (q + d / 26) % 4 == idx,
 *     sync is acquired: the assembly is cleared, this block is placed as a good block of expect = idx, the
 *     end-of-block step runs, the next judgement is at i + 27, no hit is pending. Else the hit is pending.
 *   synchronised, at i == judge_at only (one bit after the block's nominal end), the first that holds:
 *     1 nominal (bits i-26 .. i-1) matches an offset of block expect (C before C'): good, next at i + 26
 *     2 early (i-27 .. i-2) matches: good, a slip, next at i + 25
 *     3 late (i-25 .. i) matches: good, a slip, next at i + 27
 *     4 syndrome(nominal) ^ offset word is in the table: the word is corrected; bad_run stays; next at i + 26
 *     5 bad: bad_run + 1, next at i + 26; bad_run == loss_blocks: sync is lost, the pending hit and the
 *       assembly are cleared and the end-of-block step does not run
 *     (1-3 set bad_run = 0 and the block's bit in ok; 4 sets it in ok and corrected)
 *   end of block: expect == 3 with ok != 0 emits a group; expect == 3 clears the assembly; expect + 1 mod 4.
 * A call: nbits[ch] in 0 .. SDR_MAX_BITS consumes that many 0/1 bytes of the channel's row; -1, and
 * anything else but SDR_NBITS_POISONED, consumes nothing and changes nothing; SDR_NBITS_POISONED (bits are
 * missing) drops sync if there is one (lost + 1) and clears the pending hit and the assembly. The result
 * does not depend on how a channel's stream is cut into calls. */
#define SDR_RDS_MAX_GROUPS 4     /* per channel and call (256 bits hold at most three) */
typedef struct sdr_rds_group {   /* 16 bytes */
    uint16_t w[4];               /* the information words of blocks A..D, 0 where the block is not in ok */
    uint8_t ok, corrected;       /* bit b: block b was received (ok), by correction (corrected) */
    uint8_t flags;               /* SDR_RDS_GROUP_CPRIME */
    uint8_t reserved;            /* 0 */
    uint32_t bits;               /* the low 32 bits of the count of bits consumed when it was emitted */
} sdr_rds_group;
#define SDR_RDS_GROUP_CPRIME 0x1 /* block C carried offset C' */
typedef struct sdr_rds_stats {   /* 32 bytes */
    uint32_t good, corrected, bad, slips, acquired, lost, groups, synced;
} sdr_rds_stats;
typedef struct sdr_rds_opts {
    int max_burst, loss_blocks;  /* 0..5, 1..64 */
} sdr_rds_opts;
void sdr_rds_opts_default(sdr_rds_opts *o);   /* 2, 8 */
/* host only, no GPU */
uint32_t sdr_rds_syndrome(uint32_t w26);
/* tab1024 may be NULL; *entries = the number of patterns */
int sdr_rds_correction_table(int max_burst, uint32_t *tab1024, int *entries);
/* 1 when the mode's RDS chain recovers bits at 1187.5 bit/s -- its baseband rate if_Fs 247 / 640 is
 * 2375 symbol_Fs samples a second: mode 0 -- and 0 otherwise (modes 1 to 3, whose bits carry no groups) */
int sdr_rds_mode_ok(int mode);
/* host only, no GPU: SDR_OK when sdr_rds_dec_create takes the record, else SDR_E_INVALID and sdr_last_error */
int sdr_rds_opts_check(const sdr_rds_opts *opts);
/* device: the decoder is its own handle, like the meter. sdr_rds_groups enqueues one kernel (one wave per
 * channel) on `stream`; nbits_dev [nch] int32 and bits_dev [nch][bits_stride] are device arrays of
 * sdr_rds_bits' layout, ordered before it by the caller (the same stream does). Each call overwrites the
 * handle's groups [nch][SDR_RDS_MAX_GROUPS] and ngroups [nch]; the _read calls copy them (or the counters)
 * to the host and synchronise `stream`. SDR_E_INVALID, nothing enqueued: NULL handles or pointers, nch < 1,
 * options out of range, bits_stride < SDR_MAX_BITS. */
typedef struct sdr_rds_dec sdr_rds_dec;
int sdr_rds_dec_create(sdr_rds_dec **out, int device, int nch, const sdr_rds_opts *opts);
int sdr_rds_dec_destroy(sdr_rds_dec *d);
int sdr_rds_dec_reset(sdr_rds_dec *d, void *stream);
int sdr_rds_groups(sdr_rds_dec *d, const int32_t *nbits_dev, const uint8_t *bits_dev, size_t bits_stride, void *stream);
int sdr_rds_groups_read(sdr_rds_dec *d, sdr_rds_group *host_groups, int32_t *host_ngroups, void *stream);
int sdr_rds_stats_read(sdr_rds_dec *d, sdr_rds_stats *host_stats, void *stream);
/* sdr_rds_groups_read without the synchronisation, for a caller that orders the copies with an event of
 * its own (the receiver engine); the host buffers should be pinned */
int sdr_rds_groups_copy(sdr_rds_dec *d, sdr_rds_group *host_groups, int32_t *host_ngroups, void *stream);

/* The text layer (host only, plain C++, no GPU): what a station says, from its group records. A block is
 * used only when its ok bit is set. PI: block A, reported once two groups in a row agree. PTY, TP: block B.
 * Groups 0A/0B: TA, MS, and with block D the PS segment (complete when all four segments were seen since a
 * seen segment last changed); 0A's block C holds two AF codes: 1..204 = 87.6 + 0.1 code MHz, 224..249 the
 * list length (a new list), others ignored; up to 25 frequencies. 2A/2B: RadioText of 64 / 32 characters
 * (2A: blocks C and D, 2B: D), cleared when the A/B flag changes, ended by 0x0D. 4A: clock time, MJD to
 * y-m-d by the standard's formula, UTC hour and minute, local offset in half hours. Other group types are
 * counted only. Characters 0x20..0x7E are ASCII, everything else prints as '.' (the upper half of the RDS
 * character table is out of scope). */
typedef struct sdr_rds_station {
    uint16_t pi, pi_last;
    uint8_t pi_valid, pi_seen;           /* pi_valid: pi is reported; pi_seen: pi_last holds a value */
    uint8_t pty, tp, ta, ms, have_b, have_0;
    uint8_t ps[8], ps_seen, ps_complete; /* ps_seen: segment mask */
    uint8_t ps_done[8];                  /* the last complete name */
    uint8_t rt[64], rt_ab, rt_have_ab, rt_len;   /* rt_len: 64 or 32 by the last 2A / 2B */
    uint64_t rt_seen;                    /* character mask */
    uint8_t ct_valid, ct_hour, ct_minute, ct_month, ct_day;
    int8_t ct_offset;                    /* half hours, signed */
    int32_t ct_year, ct_mjd;
    uint8_t af_n, af_expect;             /* frequencies held, the list length last announced */
    uint16_t af[25];                     /* in 100 kHz: 876 + code */
    uint32_t hist[32];                   /* groups by type: 2 * type + version (needs block B) */
    uint32_t ngroups;
    uint32_t good, corrected, bad, slips, acquired, lost;   /* sdr_rds_station_stats */
} sdr_rds_station;
void sdr_rds_station_init(sdr_rds_station *s);
void sdr_rds_station_update(sdr_rds_station *s, const sdr_rds_group *g);
void sdr_rds_station_stats(sdr_rds_station *s, const sdr_rds_stats *st);
/* BLER = bad / (good + corrected + bad), 0 with no blocks */
double sdr_rds_station_bler(const sdr_rds_station *s);
/* the RBDS programme-type name the receiver prints (rds.cpp's table) */
const char *sdr_rds_pty_name(int pty);
/* a multi-line report into buf (always terminated when n > 0); returns the length it needs */
size_t sdr_rds_station_format(const sdr_rds_station *s, char *buf, size_t n);

/* ---- RDS symbol tracker (no reference counterpart; sdr_version stays 3, callers detect it by symbol): a
 * bit clock that runs on from call to call and a biphase correlator over the whole bit, in place of the
 * per-block cdr() and one-sample slicer of sdr_rds_bits. It reads rds_clean rows ([nch][stride] f32, n
 * samples a call, as sdr_rds_dsp hands them out) and writes nbits [nch] and bits [nch][bits_stride], 0/1
 * bytes, differentially decoded, in sdr_rds_bits' layout: sdr_rds_groups takes them unchanged. Mode 0 only
 * (sdr_rds_mode_ok): S = symbol_Fs = 39 samples a chip, B = 2 S = 78 a bit. One quantisation, then all
 * integer; tests/rds_track_model.py defines every bit, DESIGN.md section 4h explains the constants.
 * Per channel, with t the index of a sample in the stream since the last reset or poisoned call:
 *   quantise   q = rint(clamp(x * 2^qshift, +-32767)), round to nearest even, int32 (the bounds are integers, so
 *              this is clamp(rint(..)) too, and a product that overflows is clamped). (120 + 19712) * 32767 <
 *              2^31: every prefix sum over a call's samples and the carried ones fits int32, and so does
 *              every accumulator below (78 * 32767 * 64 < 2^31).
 *   correlator c(t) = sum q[t .. t+S-1] - sum q[t+S .. t+B-1]
 *   acquire    every t < acquire_bits * B adds |c(t)| to E[t mod B] (once sample t + B - 1 is in); after the
 *              last of them the first maximum of E is the phase, the first bit starts at
 *              t = acquire_bits * B + phase, the previous raw bit is 0. No bits while acquiring.
 *   track      the bit at t is decided in the call in which sample t + B arrives: raw = c(t) > 0,
 *              bit = raw ^ previous raw, t += B. |c(t-1)|, |c(t)|, |c(t+1)| and |c(t-S)| go to the sums
 *              early, on, late and half. After SDR_RDS_TRACK_T bits: level = on; on and half are added to the
 *              half check's sums; then, the first that holds:
 *                it is the (half_bits / T)-th round since the half check last ran and its half sum > its on
 *                  sum:                        t += S, half_moves + 1
 *                early > on and early >= late: t -= 1, moves + 1
 *                late > on:                    t += 1, moves + 1
 *              and the sums start again (the half check's only after its half_bits).
 *              c(t-S) is the half-bit correlator c(t'+S) of the bit before (t' = t - B): that one ends S - 1
 *              samples after its own bit is decided, so it is taken one bit late, when its samples are in.
 *   state      the last SDR_RDS_TRACK_CARRY quantised samples (>= B + S + 1, what the oldest undecided bit's
 *              correlators reach back to), the B accumulators, the sums. No block-sized buffer.
 * A call: n = 0 is legal and changes nothing (nbits = 0). A non-finite sample anywhere in the channel's n
 * gives nbits = SDR_NBITS_POISONED, uses none of the call's samples, and puts the channel back to acquiring
 * with an empty stream (resets + 1; the counters stay). Bits are at least B - 1 samples apart, so n <=
 * SDR_RDS_TRACK_MAX_N keeps nbits <= SDR_MAX_BITS; a larger n is refused. The result does not depend on how
 * a channel's stream is cut into calls.
 * SDR_E_INVALID, nothing enqueued: NULL handles or pointers, nch < 1, a mode sdr_rds_mode_ok refuses,
 * options out of range, n < 0 or > SDR_RDS_TRACK_MAX_N, clean_stride < n, bits_stride < SDR_MAX_BITS. */
#define SDR_RDS_TRACK_T 16        /* bits per early/late decision */
#define SDR_RDS_TRACK_CARRY 120   /* quantised samples kept between calls */
#define SDR_RDS_TRACK_MAX_N 19712 /* (SDR_MAX_BITS - 1) * (B - 1) + B - 1 */
typedef struct sdr_rds_track_stats {   /* 32 bytes */
    uint32_t locked;              /* 1: tracking, 0: acquiring */
    uint32_t phase;               /* the next bit's start mod B (0 while acquiring) */
    uint32_t bits;                /* bits emitted since the last reset */
    uint32_t moves, half_moves;   /* +-1 sample steps, S sample steps */
    uint32_t resets;              /* poisoned calls */
    uint32_t level;               /* the last round's on-time sum: T bits of |c(t)| */
    uint32_t acquired;            /* acquisitions completed */
} sdr_rds_track_stats;
typedef struct sdr_rds_track_opts {
    int qshift;                   /* 0..15 */
    int acquire_bits;             /* 1..64 */
    int half_bits;                /* a multiple of SDR_RDS_TRACK_T in T..64 */
} sdr_rds_track_opts;
void sdr_rds_track_opts_default(sdr_rds_track_opts *o);   /* 10, 32, 64 */
/* host only, no GPU: SDR_OK when sdr_rds_track_create takes the record in `mode` */
int sdr_rds_track_opts_check(int mode, const sdr_rds_track_opts *opts);
typedef struct sdr_rds_track sdr_rds_track;
int sdr_rds_track_create(sdr_rds_track **out, int device, int nch, int mode, const sdr_rds_track_opts *opts);
int sdr_rds_track_destroy(sdr_rds_track *t);
int sdr_rds_track_reset(sdr_rds_track *t, void *stream);
/* one kernel (one wave per channel) on `stream`, ordered behind the producer of clean_dev by the caller */
int sdr_rds_track_bits(sdr_rds_track *t, const float *clean_dev, size_t clean_stride, int n, int32_t *nbits_dev,
                       uint8_t *bits_dev, size_t bits_stride, void *stream);
/* host [nch]; synchronises `stream` */
int sdr_rds_track_stats_read(sdr_rds_track *t, sdr_rds_track_stats *host_stats, void *stream);

/* ---- RDS soft decisions (no reference counterpart; callers detect them by symbol): the tracker's per-bit
 * reliabilities and a Chase step of the group decoder over the least reliable raw decisions of a failing
 * block. Additive: every call above keeps its results. All integer; tests/rds_soft_model.py defines every
 * bit, DESIGN.md section 4i explains the rules.
 * Tracker: sdr_rds_track_bits_soft is sdr_rds_track_bits (the same state, clock, nbits, bits and stats) that
 *   also writes soft [nch][soft_stride] u16: soft[k] = |c(t)| >> 6 of raw decision k, the one whose XOR with
 *   raw k-1 is bit k (78 * 32767 >> 6 = 39934: no clamp). A poisoned call writes no soft values.
 * Decoder: a handle of sdr_rds_dec_create_soft takes sdr_rds_groups_soft, a handle of sdr_rds_dec_create
 *   sdr_rds_groups, and each refuses the other call. soft_bits = L in 0..6; L = 0 decodes like
 *   sdr_rds_groups bit for bit. The handle keeps the soft values of the last 32 bits a channel consumed. At a
 *   judgement at bit i, between steps 3 and 4 of the list above, on the nominal word only:
 *     candidates  the 27 raw decisions i-27 .. i-1 stand behind diff bits i-26 .. i-1; the L of them with the
 *                 smallest (soft, position), older first on ties
 *     patterns    m = 1 .. 2^L - 1 flips the candidates whose bit is set in m (bit j: the j-th candidate in
 *                 that order); a flipped raw r toggles diff bits r and r+1, clipped to the window, so the two
 *                 edge raws toggle one bit each; e(m) is the XOR, never 0
 *     weight      w(m) = the sum of the flipped candidates' soft (< 2^19)
 *     acceptance  of all m whose nominal ^ e(m) matches an offset of block expect (C before C'), the smallest
 *                 (w, m) wins
 *     effect      as step 4: the word is placed, its bit goes into ok and corrected, corrected + 1, bad_run
 *                 stays, next at i + 26; its bit also goes into the group's flags at SDR_RDS_GROUP_SOFT_SHIFT;
 *                 soft_blocks + 1, soft_flips + popcount(m). No m matches: steps 4 and 5 as above.
 *   A call consumes nbits soft values with its bits; -1 and invalid nbits consume nothing; SDR_NBITS_POISONED
 *   as above. No judgement's window reaches across a reset, a loss of sync or a poisoned call: sync is
 *   dropped and the pending hit cleared there, and the first window after an acquisition at bit i is i .. i+26.
 *   The result does not depend on how a channel's stream is cut into calls.
 * SDR_E_INVALID, nothing enqueued: as for the calls above, and NULL soft_dev, soft_stride < SDR_MAX_BITS,
 * soft_bits outside 0..6, the wrong kind of handle. */
#define SDR_RDS_GROUP_SOFT_SHIFT 4   /* sdr_rds_group.flags bit 4 + b: block b was placed by the soft step */
#define SDR_RDS_SOFT_HISTORY 32      /* soft values kept per channel between calls (>= 28) */
typedef struct sdr_rds_soft_opts {
    int max_burst, loss_blocks;  /* as sdr_rds_opts */
    int soft_bits;               /* 0..6 */
} sdr_rds_soft_opts;
void sdr_rds_soft_opts_default(sdr_rds_soft_opts *o);   /* 2, 8, 6 */
/* host only, no GPU: SDR_OK when sdr_rds_dec_create_soft takes the record */
int sdr_rds_soft_opts_check(const sdr_rds_soft_opts *opts);
typedef struct sdr_rds_soft_stats {   /* 16 bytes */
    uint32_t soft_blocks;        /* blocks placed by the soft step (they count in sdr_rds_stats.corrected too) */
    uint32_t soft_flips;         /* raw decisions flipped in them */
    uint32_t soft_bits;          /* the handle's option */
    uint32_t reserved;           /* 0 */
} sdr_rds_soft_stats;
int sdr_rds_track_bits_soft(sdr_rds_track *t, const float *clean_dev, size_t clean_stride, int n, int32_t *nbits_dev,
                            uint8_t *bits_dev, size_t bits_stride, uint16_t *soft_dev, size_t soft_stride, void *stream);
int sdr_rds_dec_create_soft(sdr_rds_dec **out, int device, int nch, const sdr_rds_soft_opts *opts);
int sdr_rds_groups_soft(sdr_rds_dec *d, const int32_t *nbits_dev, const uint8_t *bits_dev, size_t bits_stride,
                        const uint16_t *soft_dev, size_t soft_stride, void *stream);
/* host [nch]; synchronises `stream`; a handle of sdr_rds_dec_create reads as zeros */
int sdr_rds_soft_stats_read(sdr_rds_dec *d, sdr_rds_soft_stats *host_stats, void *stream);

/* ---- RDS carrier-phase derotator (no reference counterpart; callers detect it by symbol): the reference's
 * RDS chain demodulates with a carrier that sits at an unexplained, roughly constant angle (about 45 degrees)
 * off the 57 kHz subcarrier, so its rds_clean row holds only part of the RDS power. Given that row and the same
 * chain run with the quadrature carrier, this stage estimates the angle from the squared signal, window by
 * window, and turns both rows onto one axis: out = Re((I + jQ) e^{-j phi}), rows the tracker reads as it reads
 * rds_clean. Mode 0 only (sdr_rds_mode_ok). One quantisation, then all integer: no libm and no floating point
 * after it; tests/rds_carrier_model.py defines every bit, DESIGN.md section 4j explains the constants.
 * Per channel, with t the index of a sample in the stream since the last reset or poisoned call:
 *   quantise   qi, qq = rint(clamp(x * 2^qshift, +-32767)) of the two rows, as the tracker quantises
 *   rotate     y = clamp((qi c + qq s + 2^13) >> 14, +-32767), out = y * 2^-qshift as f32, which is exact: the
 *              tracker's own quantisation (same qshift) gets y back. |qi c + qq s| <= 32767 * 23173 < 2^31.
 *   window     (c, s) is constant over a window of SDR_RDS_CARRIER_W samples of the stream (not of the call)
 *              and (2^14, 0) in the first one
 *   phasor     at the end of a window: Pr = sum(qi^2 - qq^2), Pi = sum(2 qi qq), Pt = sum(qi^2 + qq^2) over
 *              its samples, int64: a term is below 2^31, a sum at most W * 2^31 = 2^42. Then
 *              Sr += (Pr - Sr) >> avg_shift, Si and St likewise, the shift arithmetic: S stays between its old
 *              value and P, so |S| <= 2^42 too.
 *   angle      with m = max(|Sr|, |Si|) > 0, Sr and Si are shifted by the same count, right (arithmetic) or
 *              left, that puts m into [2^28, 2^29). A vectoring CORDIC of SDR_RDS_CARRIER_CORDIC_N = 24
 *              iterations on int32 gives the angle of (x, y), an int32 with a turn = 2^32:
 *                z = 0; x < 0: (x, y, z) = (-x, -y, 2^31)
 *                i = 0 .. 23:  y >= 0: (x, y, z) = (x + (y >> i), y - (x >> i), z + A[i])
 *                              else:   (x, y, z) = (x - (y >> i), y + (x >> i), z - A[i])
 *              A[i] = round(atan(2^-i) / 2 pi * 2^32) = 536870912, 316933406, 167458907, 85004756, 42667331,
 *              21354465, 10679838, 5340245, 2670163, 1335087, 667544, 333772, 166886, 83443, 41722, 20861,
 *              10430, 5215, 2608, 1304, 652, 326, 163, 81. (x grows by 1.6468: below 2^29.5 * 1.6468 < 2^31.)
 *              phi = z >> 1 (arithmetic); if |wrap32(phi - phi_prev)| > 2^30, phi += 2^31 (wrapping): of the
 *              two answers half a turn apart, the one nearer the last. m = 0 keeps phi and (c, s).
 *   vector     (c, s) of the next window by the rotation CORDIC: z = phi; |z| > 2^30: z -= 2^31 (wrapping) and
 *              the result is negated; (x, y) = (326016437, 0) (2^29 over the CORDIC's gain);
 *                i = 0 .. 23:  z >= 0: (x, y, z) = (x - (y >> i), y + (x >> i), z - A[i])
 *                              else:   (x, y, z) = (x + (y >> i), y - (x >> i), z + A[i])
 *              c = (x + 2^14) >> 15, s = (y + 2^14) >> 15.
 *   state      the partial sums and length of the current window, S, phi, (c, s), the counters. No samples.
 * A call: n = 0 is legal and changes nothing. A non-finite sample in either row within the channel's n writes
 * NaN to all n samples of its output row (the tracker behind it then reports SDR_NBITS_POISONED), uses none of
 * the call's samples and puts the channel back to its first window (phi = 0, S = 0; resets + 1, windows
 * stays). The result does not depend on how a channel's stream is cut into calls. The output rows must not
 * overlap the input rows.
 * SDR_E_INVALID, nothing enqueued: NULL handles or pointers, nch < 1, a mode sdr_rds_mode_ok refuses, options
 * out of range, n < 0 or > SDR_RDS_TRACK_MAX_N, a stride < n, a pointer that is not a float's. */
#define SDR_RDS_CARRIER_W 2048        /* samples of the stream per window */
#define SDR_RDS_CARRIER_CORDIC_N 24
typedef struct sdr_rds_carrier_stats {   /* 40 bytes */
    int64_t sr, si, st;           /* the smoothed phasor of the squared signal and the smoothed power */
    int32_t phi;                  /* the phase in use, a turn = 2^32: degrees = phi * 360 / 2^32 */
    uint32_t windows;             /* windows completed since the last reset */
    uint32_t resets;              /* poisoned calls */
    uint32_t reserved;            /* 0 */
} sdr_rds_carrier_stats;          /* coherence = hypot(sr, si) / st: 1 for a clean BPSK subcarrier, near 0 for noise */
typedef struct sdr_rds_carrier_opts {
    int qshift;                   /* 0..15; the tracker behind it wants the same */
    int avg_shift;                /* 0..6: S += (P - S) >> avg_shift */
} sdr_rds_carrier_opts;
void sdr_rds_carrier_opts_default(sdr_rds_carrier_opts *o);   /* 10, 3 */
/* host only, no GPU: SDR_OK when sdr_rds_carrier_create takes the record in `mode` */
int sdr_rds_carrier_opts_check(int mode, const sdr_rds_carrier_opts *opts);
typedef struct sdr_rds_carrier sdr_rds_carrier;
int sdr_rds_carrier_create(sdr_rds_carrier **out, int device, int nch, int mode, const sdr_rds_carrier_opts *opts);
int sdr_rds_carrier_destroy(sdr_rds_carrier *h);
int sdr_rds_carrier_reset(sdr_rds_carrier *h, void *stream);
/* one kernel (one wave per channel) on `stream`: clean_i, clean_q [nch][stride] f32 in, out [nch][out_stride] */
int sdr_rds_carrier_rotate(sdr_rds_carrier *h, const float *clean_i, size_t stride_i, const float *clean_q,
                           size_t stride_q, int n, float *out, size_t out_stride, void *stream);
/* host [nch]; synchronises `stream` */
int sdr_rds_carrier_stats_read(sdr_rds_carrier *h, sdr_rds_carrier_stats *host_stats, void *stream);

/* mono loop body (mono.cpp:34-42) on the current block: audio [nch][n_audio] int16 */
int sdr_mono(sdr_ctx *ctx, int16_t *audio, size_t audio_stride, void *stream);
/* stereo loop body (stereo.cpp:74-107): lr [nch][2*n_audio] int16, L/R interleaved */
int sdr_stereo(sdr_ctx *ctx, int16_t *lr, size_t lr_stride, void *stream);
/* rds DSP (rds.cpp:105-133): rds_clean [nch][n_rds] f32 (may be NULL: kept internally) */
int sdr_rds_dsp(sdr_ctx *ctx, float *rds_clean, size_t rds_stride, void *stream);
/* The same two loop bodies split at their PLL, in this order per block (each part may run on its
 * own stream; the caller orders them with events): sdr_X = sdr_X_pre; sdr_X_pll; sdr_X_post.
 *   stereo_pre   pilot + band BPFs          stereo.cpp:74, :80
 *   stereo_pll   19 kHz PLL, x2 carrier      stereo.cpp:77
 *   stereo_post  mixer, delay, resamplers    stereo.cpp:83-107
 *   rds_pre      BPF, squaring, 114 kHz BPF  rds.cpp:105-116
 *   rds_pll      114 kHz PLL, x0.5           rds.cpp:119
 *   rds_post     delay, mixer, 247/640, RRC  rds.cpp:122-133
 * Intermediates crossing the split are kept per block parity, so the PLL of block b+1 may run
 * while block b's post part is still running. Parity release (threadsafequeue.h:29-31): the
 * readers of a block's parity buffers -- sdr_mono, sdr_stereo_post and sdr_rds_post's mixer --
 * record on their stream that they have read it, and sdr_frontend (likewise sdr_push_fm_demod,
 * the pre parts and sdr_frontend_pre_parts) waits on its own stream until the readers of block
 * b-2, which used the same parity, have done so: the caller needs no wait of its own for that
 * reuse. Outputs handed to the caller (lr, rds_clean, bits) are the caller's to order. The wait is
 * bounded (5 s): a reader that has not released its block by then makes it an error, never wrong
 * output -- the producer goes on, every output stage that runs afterwards writes SDR_PCM_POISON
 * audio (mono and stereo), NaN rds_clean rows and nbits = SDR_NBITS_POISONED, and every later call
 * on the context returns SDR_E_TIMEOUT until sdr_ctx_reset. */
int sdr_stereo_pre(sdr_ctx *ctx, void *stream);
int sdr_stereo_pll(sdr_ctx *ctx, void *stream);
int sdr_stereo_post(sdr_ctx *ctx, int16_t *lr, size_t lr_stride, void *stream);
int sdr_rds_pre(sdr_ctx *ctx, void *stream);
/* sdr_stereo_pre + sdr_rds_pre of the current block on ONE stream: the pilot, band and RDS band
 * BPFs read the staged fm_demod window once (stereo.cpp:74,80 and rds.cpp:105 share the input),
 * then the squared-RDS BPF. For callers that run both pre parts on the same stream. */
int sdr_pre(sdr_ctx *ctx, void *stream);
int sdr_rds_pll(sdr_ctx *ctx, void *stream);
int sdr_rds_post(sdr_ctx *ctx, float *rds_clean, size_t rds_stride, void *stream);
/* stereo_pll + rds_pll of the current block in one dispatch (2 x nch independent recurrences);
 * needs both _pre parts done. */
int sdr_plls(sdr_ctx *ctx, void *stream);
/* Persistent PLLs: the stereo + RDS PLLs of many consecutive blocks in ONE dispatch (no launch
 * gap between blocks). sdr_plls_launch(nblocks) on the PLL stream, before the sdr_frontend of the
 * first of those blocks; then per block, after both _pre parts, sdr_plls_signal on the stream that
 * ran them (instead of sdr_plls) and sdr_plls_wait on the stream of the _post parts. The kernel
 * waits for each block's signal (a device flag written in stream order), runs both PLLs, and
 * releases the waiting stream. The PLL stream must be one sdr_stream_create_cu_range made (it owns
 * its hardware queue; on a pool stream a signal could queue behind the waiting launch), and every
 * workgroup of the launch must be resident on that stream's CUs at once -- by the workgroups of its
 * kernel that fit one CU and by how the CU mask falls on the XCCs' shader engines (workgroups are
 * dealt to the engines evenly, so an engine with fewer CUs of the mask fills first; sdr_plls_fits):
 * otherwise the launch is refused with SDR_E_INVALID before anything is enqueued (use sdr_plls, or
 * another CU range). A wait longer than 5 s (a block
 * never signalled, or a post stream that waits for a block the PLL never finished) ends the launch
 * without computing: from then on the post stages of that launch's blocks write SDR_PCM_POISON
 * audio, NaN rds_clean rows and nbits = SDR_NBITS_POISONED (never audio from phases the PLL did
 * not produce), sdr_plls_report returns SDR_E_HIP, and after that report the post calls of those
 * blocks fail too; sdr_ctx_reset + a new launch recover. sdr_plls_report also returns each
 * block's PLL time of the last launch (ms, from the device clock: its last wave's end minus the
 * later of its signal and the previous block's end) and synchronises `stream`. While a launch still
 * waits for blocks, nothing may synchronise with the PLL stream implicitly: a CU-masked stream is a
 * blocking stream, so work on the legacy null stream would wait for it (until the 5 s bound). Each
 * block must be waited for (sdr_plls_wait) before the 16th block after it is signalled. Launching
 * again while blocks of the previous launch were never signalled first lets that launch time out
 * and drain. Not with SDR_FLAG_PLL_LIBM. */
int sdr_plls_launch(sdr_ctx *ctx, int nblocks, void *stream);
/* The same for one of the two PLLs (which = SDR_PLLS_STEREO or SDR_PLLS_RDS; SDR_PLLS_BOTH is
 * sdr_plls_launch): for a context that runs one chain only, as each consumer thread of the reference
 * does (project.cpp:134-136: stereo in the audio thread, RDS in the rds thread). sdr_plls_signal
 * then needs only that chain's _pre part, and only that chain's _post part follows the wait. */
#define SDR_PLLS_STEREO 1
#define SDR_PLLS_RDS 2
#define SDR_PLLS_BOTH 3
int sdr_plls_launch_sel(sdr_ctx *ctx, int nblocks, int which, void *stream);
/* Would sdr_plls_launch_sel(which) accept a stream made by sdr_stream_create_cu_range(first_cu, n_cu,
 * exclude = 0) for this context? Fills the launch's waves, its workgroups and how many of them that
 * CU range keeps resident at once; it fits when *groups <= *resident. No stream is made, nothing is
 * enqueued. */
int sdr_plls_fits(sdr_ctx *ctx, int which, int first_cu, int n_cu, int *waves, long long *groups,
                  long long *resident);
/* Optional, ahead of sdr_plls_launch(nblocks) (e.g. before a timed region): the launch's
 * bookkeeping -- allocation, the reset of its stamps and error word -- in `stream`'s order, so the
 * launch itself only enqueues the kernel. Ignored by a launch with another nblocks. */
int sdr_plls_prepare(sdr_ctx *ctx, int nblocks, void *stream);
int sdr_plls_signal(sdr_ctx *ctx, void *stream);
/* The pipeline fill: the FIRST block of a pending persistent launch as sdr_frontend + sdr_pre +
 * sdr_plls_signal in `nparts` sample ranges (at most one per 2048-sample pre-PLL FIR tile), each
 * range published as soon as its front end and pre-PLL FIRs are done, so the PLLs start on the
 * block's first range while the rest is produced (the reference's producer hands a block over whole,
 * threadsafequeue.h:24-44; the PLL consumes its input in order, pll.cpp:34-53, and waits before
 * every sample that is not published yet). Exact numerics, rds_on, 101 taps only. */
int sdr_frontend_pre_parts(sdr_ctx *ctx, const uint8_t *iq, size_t iq_stride, int nparts, void *stream);
int sdr_plls_wait(sdr_ctx *ctx, void *stream);
int sdr_plls_report(sdr_ctx *ctx, double *block_ms, int max_blocks, int *nblocks, void *stream);
/* The raw device stamps of the last persistent launch (100 MHz s_memrealtime ticks), per block:
 * t_start[j] = when its signal was seen, t_end[j] = its last wave's end; synchronises `stream`. */
int sdr_plls_timeline(sdr_ctx *ctx, unsigned long long *t_start, unsigned long long *t_end, int max_blocks,
                      int *nblocks, void *stream);
/* Per-step cost of the last persistent launch from the waves' own clocks: shader cycles per PLL step
 * and wave (s_memtime over each wave's compute of each block, averaged) and the shader clock over
 * the same intervals (against the 100 MHz s_memrealtime); synchronises `stream`. */
int sdr_plls_cycles(sdr_ctx *ctx, double *cycles_per_step, double *clock_mhz, void *stream);
/* The same per block j < max of the last persistent launch (cycles per step and wave, shader clock);
 * *n = the launch's block count. */
int sdr_plls_block_cycles(sdr_ctx *ctx, double *cycles_per_step, double *clock_mhz, int max, int *n,
                          void *stream);
/* rds symbol/bit recovery (rds.cpp:135-167): per channel, for blocks with block_count > 5 and
 * rds_on: offset = cdr(), symbols (0/1 bytes), bits (decoded 0/1 bytes). nbits[ch] = -1 on
 * blocks that do not decode. Any output pointer may be NULL. Strides in elements. */
int sdr_rds_bits(sdr_ctx *ctx, int32_t *offset, int32_t *nsym, uint8_t *symbols, size_t sym_stride,
                 int32_t *nbits, uint8_t *bits, size_t bits_stride, void *stream);
/* Consumer-side entry (wait_and_pop, threadsafequeue.h:46): make an fm_demod block produced
 * elsewhere (another context, another GPU, or host data copied to the device) the context's
 * current block; mono/stereo/rds then consume it. fm [nch][block_if] device memory. */
int sdr_push_fm_demod(sdr_ctx *ctx, const float *fm, size_t fm_stride, void *stream);
/* Copy out the context's current-block fm_demod [nch][block_if] (the reference's queue payload) */
int sdr_get_fm_demod(sdr_ctx *ctx, float *fm, size_t fm_stride, void *stream);
/* Debug / parity access to intermediates of the current block (device pointers into the
 * context, valid until the next sdr_frontend; "carrier", "stereo_dc" and "ipll" hold whole rows only
 * with SDR_FLAG_KEEP_INTERMEDIATES): name in {"fm","pilot","carrier","band","rds_band",
 * "gen_pilot","ipll","rds_dc","rds_filt","rds_clean","stereo_dc"}; *stride in elements. Flagged rows:
 * "rds_dc_q", "rds_filt_q", "rds_clean_q" (SDR_FLAG_RDS_QUAD), "if_env" (SDR_FLAG_IF_ENVELOPE, at sdr_meter_rf). */
int sdr_ctx_buffer(sdr_ctx *ctx, const char *name, const float **ptr, size_t *stride, int *len);

/* ---- RDS quadrature branch (no reference counterpart; callers detect it by symbol). With SDR_FLAG_RDS_QUAD,
 * sdr_rds_post runs the reference's RDS chain from the mixer on a second time, with the quadrature of its
 * carrier, into rds_clean_q [nch][n_rds]; every other result of the context stays bit for bit what it is
 * without the flag. Per block of n = block_if samples, t[] the 114 kHz PLL's phases of the block:
 *     ipll_q[i]   = RN32(cos((double)(t[i-1] * 0.5f + -(float)(pi/2)))), i = 1 .. n: the reference's NCO output
 *                   (pll.cpp:52) with phaseAdjust -pi/2; ipll_q[0] is the previous block's ipll_q[n], and
 *                   0.0f in the first block and after sdr_ctx_reset
 *     rds_dc_q[i] = (2 * (rds_band[i - 50] + 0)) * ipll_q[i], i = 0 .. n-1, in f32 (rds.cpp:122-127)
 *     rds_filt_q  = the 247/640 resampler of rds.cpp:130 over rds_dc_q, rds_clean_q = the RRC of :133 over it,
 *                   with FIR states of their own (zero at the start)
 * which is fmpll(gen_pilot, 114e3, if_Fs, out_q, st_q, 0.5, -(float)(pi/2), 0.001) on a pllblock_args and a
 * zeroed out_q of its own, then the reference's mixer, resampler and RRC. A poisoned block (SDR_NBITS_POISONED
 * above) writes NaN rows to rds_clean_q as to rds_clean. The rows are also "rds_clean_q", "rds_filt_q" and
 * "rds_dc_q" of sdr_ctx_buffer. SDR_E_INVALID without the flag. */
int sdr_ctx_rds_clean_q(sdr_ctx *ctx, const float **ptr, size_t *stride, int *len);

/* Streams on disjoint CU sets (no reference counterpart: the reference's three threads,
 * project.cpp:134-136, share one CPU; this is their placement on the GPU). Creates a HIP stream
 * on `device` whose kernels run only on CU-mask bits [first_cu, first_cu + n_cu) (exclude = 0),
 * or on every CU except those (exclude = 1). Giving the serial PLL stream (sdr_plls) its own CUs
 * keeps the other stages' kernels off the SIMDs its lone waves issue from.
 * Release with sdr_stream_destroy. */
int sdr_stream_create_cu_range(void **stream, int device, int first_cu, int n_cu, int exclude);
int sdr_stream_destroy(void *stream);

/* Bandwidth calibration (no reference counterpart): device-to-device copy of `bytes` (a multiple
 * of 16, 16-byte aligned pointers) with a streaming kernel over every CU, so that a benchmark can
 * state the HBM rate a plain stream reaches next to the nominal peak. */
int sdr_hbm_copy(void *dst, const void *src, size_t bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
