// sdr_ctx.hip -- the context's lifecycle: the thread's last error, the mode table, allocation, the
// tap and polyphase tables, sdr_ctx_create / destroy / reset / info / buffer, the arguments a block's
// front end and PLLs take from the context, and the parity-release protocol between the streams that
// read a block's buffers and the ones that overwrite them.

#include "sdr_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace sdrk {
namespace {
thread_local std::string g_err;
}  // namespace

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

const char* last_error() { return g_err.c_str(); }
}  // namespace sdrk

using namespace sdrk;

namespace {

// The parity-release wait (release_wait): every word w[k] with bit k of mask reaches want[k] (counts
// stored by k_flag_store after the readers' kernels); polled relaxed, acquired once, bounded like the
// persistent PLL's waits. After ~5 s it gives up: it sets the context's sticky fail word (every output
// stage then poisons its block: a reader that runs after the producer's overwrite would read the
// next block's data) and its host-mapped mirror (the next stage call returns SDR_E_TIMEOUT) before it
// lets the stream go on, so no reader can start after the overwrite without seeing the word.
struct RelWant {
    uint32_t v[sdr_ctx::Rel::SLOTS];
};
__global__ void k_rel_wait(const uint32_t* w, const RelWant wants, unsigned mask, uint32_t* fail, uint32_t* fail_host) {
    if (threadIdx.x != 0) return;
    const uint32_t* want = wants.v;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    bool expired = false;
#pragma unroll
    for (int k = 0; k < sdr_ctx::Rel::SLOTS && !expired; k++) {
        if (!(mask & (1u << k))) continue;
        while ((int32_t)(__hip_atomic_load(w + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - want[k]) < 0) {
            __builtin_amdgcn_s_sleep(4);
            if (__builtin_amdgcn_s_memrealtime() - t0 > 500000000ull) {
                expired = true;
                break;
            }
        }
    }
    if (expired) {
        __hip_atomic_fetch_or(fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(fail_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");          // both visible before the kernel ends
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// x[ch][col] = v for every channel row (the carried last NCO sample at initialisation)
__global__ void k_set_col(float* x, size_t stride, int col, int nch, float v) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch < nch) x[(size_t)ch * stride + col] = v;
}

__global__ void k_fill_u8(uint8_t* p, uint8_t v, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

template <typename T>
int dalloc(sdr_ctx* c, T** p, size_t count) {
    void* v = nullptr;
    HIP_TRY(hipMalloc(&v, count * sizeof(T) + 256));
    HIP_TRY(hipMemset(v, 0, count * sizeof(T) + 256));
    c->allocs.push_back(v);
    *p = static_cast<T*>(v);
    return SDR_OK;
}

template <typename T>
int upload(sdr_ctx* c, T** p, const std::vector<T>& host) {
    int r = dalloc(c, p, host.size());
    if (r) return r;
    HIP_TRY(hipMemcpy(*p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return SDR_OK;
}

int init_state(sdr_ctx* c, hipStream_t s) {
    const sdr_info& in = c->info;
    // every buffer back to zero (the reference's value-initialised vectors)
    HIP_TRY(hipMemsetAsync(c->fm - HIST, 0, 2 * c->fm_par * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(c->sdc - HIST, 0, 2 * c->fm_par * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(c->rband - HIST, 0, 2 * c->fm_par * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(c->rdc - HIST, 0, 2 * c->fm_par * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(c->rfilt - HIST, 0, 2 * c->rf_par * sizeof(float), s));
    if (c->flags & SDR_FLAG_RDS_QUAD) {             // ipll_q[0] of the first block is 0.0f: a zeroed out buffer
        HIP_TRY(hipMemsetAsync(c->rdc_q - HIST, 0, 2 * c->fm_par * sizeof(float), s));
        HIP_TRY(hipMemsetAsync(c->rfilt_q - HIST, 0, 2 * c->rf_par * sizeof(float), s));
        HIP_TRY(hipMemsetAsync(c->ipll_q_last, 0, (size_t)2 * c->nch * sizeof(float), s));
    }
    const size_t tail_bytes = (size_t)2 * c->nch * 2 * (c->ntaps - 1);
    hipLaunchKernelGGL(k_fill_u8, dim3((unsigned)((tail_bytes + 255) / 256)), dim3(256), 0, s, c->tail,
                       (uint8_t)128, tail_bytes);  // u8 128 == 0.0f: zero FIR state
    LAUNCH_CHECK();
    HIP_TRY(hipMemsetAsync(c->prev, 0, (size_t)2 * c->nch * sizeof(float2), s));
    std::vector<sdr_pll_state> st(c->nch);
    for (auto& p : st) p = sdr_pll_state{1.0f, 0.0f, 0.0f, 0.0f, 0.0, 1.0f};  // stereo.cpp:51-57, :45
    HIP_TRY(hipMemcpyAsync(c->st_pll, st.data(), st.size() * sizeof(sdr_pll_state), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->rds_pll, st.data(), st.size() * sizeof(sdr_pll_state), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(c->dec, 0, (size_t)c->nch * DEC_STATE * sizeof(int32_t), s));
    // carrier[0] of the first block = lastCarrier = 1 (stereo.cpp:45): the NCO reads it from the
    // other parity's row end
    for (int p = 0; p < 2; p++) {
        hipLaunchKernelGGL(k_set_col, dim3(cdiv(c->nch, 64)), dim3(64), 0, s, c->carrier + p * c->pll_par, c->pll_stride,
                           in.block_if, c->nch, 1.0f);
        hipLaunchKernelGGL(k_set_col, dim3(cdiv(c->nch, 64)), dim3(64), 0, s, c->ipll + p * c->pll_par, c->pll_stride,
                           in.block_if, c->nch, 1.0f);
    }
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize(s));
    c->parity = 1;
    c->block = -1;
    c->stereo_done = c->rds_dsp_done = c->rds_bits_done = c->mono_done = -1;
    c->st_pre_done = c->st_pll_done = c->rds_pre_done = c->rds_pll_done = -1;
    c->env_block = -1;             // (if_env itself needs no clearing: every element is written before it is valid)
    (void)in;
    return SDR_OK;
}

}  // namespace

namespace sdrk {

int mode_info(sdr_info* in, int nch, int mode, int rds_on) {
    std::memset(in, 0, sizeof(*in));
    in->nch = nch;
    in->mode = mode;
    in->rds_on = rds_on;
    in->rf_taps = 101;
    in->rf_Fs = 2400000; in->rf_decim = 10; in->if_Fs = 240000; in->audio_upsample = 1;
    in->audio_decim = 5; in->symbol_Fs = 39;
    switch (mode) {  // project.cpp:67-108
        case 0: break;
        case 1: in->rf_Fs = 1440000; in->rf_decim = 4; in->audio_decim = 9; in->if_Fs = 360000; break;
        case 2: in->audio_decim = 800; in->audio_upsample = 147; in->symbol_Fs = 20; break;
        case 3: in->rf_Fs = 1152000; in->rf_decim = 3; in->audio_decim = 1280; in->if_Fs = 384000;
                in->audio_upsample = 147; in->symbol_Fs = 20; break;
        default: return fail(SDR_E_INVALID, "mode %d not in 0..3", mode);
    }
    const int U = in->audio_upsample, D = in->audio_decim;
    in->block_iq = (1470 * in->rf_decim * D) / U;
    in->block_if = (1470 * D) / U;
    in->n_audio = in->block_if * U / D;
    in->n_rds = in->block_if * 247 / 640;
    in->history = HIST;
    return SDR_OK;
}

Polyphase make_polyphase(const std::vector<float>& h, int U) {
    Polyphase p;
    const int ntaps = (int)h.size();
    int maxc = 0;
    p.cnt.resize(U);
    for (int ph = 0; ph < U; ph++) {
        p.cnt[ph] = ph < ntaps ? (ntaps - ph + U - 1) / U : 0;
        maxc = std::max(maxc, p.cnt[ph]);
    }
    p.L = (maxc + 3) & ~3;
    p.table.assign((size_t)U * p.L, 0.0f);
    for (int ph = 0; ph < U; ph++)
        for (int j = 0; j < p.cnt[ph]; j++) p.table[(size_t)ph * p.L + j] = h[ph + (size_t)U * j];
    return p;
}

PllJob stereo_job(sdr_ctx* c) {
    const sdr_info& in = c->info;
    return PllJob{c->plain(c->pilot), c->plain_stride, c->plain(c->t_st), c->plain_stride, c->pllbuf(c->carrier),
                  c->pll_stride, c->st_pll, 19e3f, (float)(in.rf_Fs / in.rf_decim), 0.01f, 2.0f, 0.0f,
                  c->carrier + (c->parity ^ 1) * c->pll_par, c->rxbuf(c->rx_st), c->plain_stride,
                  c->plain(c->pilot_neg), c->plain_stride};
}
PllJob rds_job(sdr_ctx* c) {
    const sdr_info& in = c->info;
    return PllJob{c->plain(c->gpilot), c->plain_stride, c->plain(c->t_rds), c->plain_stride, c->pllbuf(c->ipll),
                  c->pll_stride, c->rds_pll, 114e3f, (float)in.if_Fs, 0.001f, 0.5f, 0.0f,
                  c->ipll + (c->parity ^ 1) * c->pll_par, c->rxbuf(c->rx_rds), c->plain_stride,
                  c->plain(c->gpilot_neg), c->plain_stride};
}

FrontendArgs frontend_args(const sdr_ctx* c, const uint8_t* iq, size_t iq_stride, int p) {
    const sdr_info& in = c->info;
    const int hp = c->ntaps - 1;
    FrontendArgs a{};
    a.iq = iq;
    a.iq_stride = iq_stride;
    a.tail_in = c->tail + (size_t)(p ^ 1) * c->nch * 2 * hp;
    a.tail_out = c->tail + (size_t)p * c->nch * 2 * hp;
    a.prev_in = c->prev + (size_t)(p ^ 1) * c->nch;
    a.prev_out = c->prev + (size_t)p * c->nch;
    a.fm = c->fm + p * c->fm_par;
    a.fm_other = c->fm + (p ^ 1) * c->fm_par;
    a.fm_stride = c->fm_stride;
    a.env = c->if_env ? c->if_env + p * c->fm_par : nullptr;
    a.nch = c->nch;
    a.ntaps = c->ntaps;
    a.block_iq = in.block_iq;
    a.block_if = in.block_if;
    a.D = in.rf_decim;
    a.h = c->rf_h;
    a.hs = c->rf_hs;
    a.afrag = c->fe_afrag;
    a.yscale = c->fe_yscale;
    a.pad80 = c->pad80;
    a.fast = (c->flags & SDR_FLAG_FAST_FRONTEND) != 0 && c->fe_afrag != nullptr;
    a.phase = (c->flags & SDR_FLAG_PHASE_DEMOD) != 0;
    return a;
}

// Parity release across streams (threadsafequeue.h:29-31: a producer reuses a buffer only after its
// consumers released it). The block of parity p is read by the mono stage, the stereo post stage and
// the RDS mixer; each stores the count of blocks of that parity it has read into a device word on its
// stream after its kernels that read them (k_flag_store, ordered after them), and the stages that
// overwrite parity p two blocks later wait on their stream for the count the host last enqueued
// (k_flag_wait) -- unless that reader ran on the same stream, whose order already holds. Slots:
// REL_MONO (fm), REL_STEREO (fm, band, t_st, carrier), REL_RDS (rband, t_rds, ipll). Device words,
// not HIP events: a cross-stream event wait between the CU-masked streams started the waiting
// stream 60-200 us after the event's work had completed (profiles/r04/release/), a kernel poll
// within a few us.
// The reception meter's calls are readers too (sdr_meter.hip): REL_METER_A sdr_meter_audio (fm, pilot),
// REL_METER_R sdr_meter_rds (rband) -- a slot each, because the two may run on different streams and a
// slot's word is stored, not added to. On a context no meter call ran on their counts stay 0 and
// release_wait skips them: such a context enqueues what it always did. REL_METER_RF sdr_meter_rf (if_env) is the
// third such reader, with a slot of its own for the same reason; only the front ends overwrite its row.
int release_record(sdr_ctx* c, unsigned slot, hipStream_t s) {
    sdr_ctx::Rel& r = c->rel;
    const int p = c->parity, k = __builtin_ctz(slot);
    r.seq[p][k]++;
    r.stream[p][k] = s;
    return launch_flag_store(r.words + p * sdr_ctx::Rel::SLOTS + k, r.seq[p][k], s);
}
int release_wait(sdr_ctx* c, int p, unsigned slots, hipStream_t s) {
    sdr_ctx::Rel& r = c->rel;
    unsigned mask = 0;
    for (int k = 0; k < sdr_ctx::Rel::SLOTS; k++) {
        const uint32_t want = r.seq[p][k];
        if (!(slots & (1u << k)) || want == 0 || r.stream[p][k] == s ||
            (r.waited_on[p][k] == s && r.waited[p][k] == want))
            continue;
        mask |= 1u << k;
        r.waited[p][k] = want;
        r.waited_on[p][k] = s;
    }
    if (!mask) return SDR_OK;
    RelWant wants;
    for (int k = 0; k < sdr_ctx::Rel::SLOTS; k++) wants.v[k] = r.seq[p][k];
    hipLaunchKernelGGL(k_rel_wait, dim3(1), dim3(64), 0, s, r.words + p * sdr_ctx::Rel::SLOTS, wants, mask,
                       r.fail_words, r.fail_host_dev);
    LAUNCH_CHECK();
    return SDR_OK;
}
// a parity-release wait of this context gave up (k_rel_wait set the host-mapped fail word): every
// stage call fails until sdr_ctx_reset (the device poisons the outputs of the stages already queued)
int check_failed(const sdr_ctx* c, const char* what) {
    if (c->rel.fail_host && __atomic_load_n(c->rel.fail_host, __ATOMIC_ACQUIRE) != 0u)
        return fail(SDR_E_TIMEOUT, "%s: a parity-release wait timed out (a reader did not release its block within "
                                   "5 s, and the producer overwrote it): outputs since are poisoned; sdr_ctx_reset",
                    what);
    return SDR_OK;
}

}  // namespace sdrk

extern "C" {

const char* sdr_last_error(void) { return sdrk::last_error(); }
int sdr_version(void) { return 3; }   // 2: the shared-capture tuner (sdr_tuner_*, sdr_frontend_tuned); 3: the band scan (sdr_scan_*)

int sdr_ctx_create(sdr_ctx** out, int device, int nch, int mode, int rds_on, int flags) {
    if (!out || nch <= 0) return fail(SDR_E_INVALID, "bad arguments");
    *out = nullptr;
    if ((flags & SDR_FLAG_FAST_FRONTEND) && (flags & SDR_FLAG_PHASE_DEMOD))
        return fail(SDR_E_INVALID, "SDR_FLAG_PHASE_DEMOD needs the exact front end (not SDR_FLAG_FAST_FRONTEND)");
    if ((flags & SDR_FLAG_FAST_FRONTEND) && (flags & SDR_FLAG_IF_ENVELOPE))
        return fail(SDR_E_INVALID, "SDR_FLAG_IF_ENVELOPE needs the exact front end (not SDR_FLAG_FAST_FRONTEND)");
    if ((flags & SDR_FLAG_RDS_QUAD) && !(rds_on && sdr_rds_mode_ok(mode)))
        return fail(SDR_E_INVALID, "SDR_FLAG_RDS_QUAD needs rds_on and mode 0 (mode %d, rds_on %d)", mode, rds_on);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0)
        return fail(SDR_E_NODEV, "no HIP device %d", device);
    HIP_TRY(hipSetDevice(device));
    sdr_ctx* c = new sdr_ctx();
    c->device = device;
    c->nch = nch;
    c->mode = mode;
    c->rds_on = rds_on ? 1 : 0;
    c->flags = flags;
    {
        int cus = 0;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
        c->cus = cus;
    }
    int r = mode_info(&c->info, nch, mode, c->rds_on);
    if (r) { delete c; return r; }
    const sdr_info& in = c->info;
    const int T = in.rf_taps, U = in.audio_upsample;
    c->ntaps = T;
    // ---- taps (host design, reference formulas) ----
    std::vector<float> rf(T), audio((size_t)T * U), pilot(T), stereo(T), rds(T), rds_sq(T), rdsbb((size_t)T * 247),
        rrc(T);
    const float fb_pilot[2] = {18.5e3f, 19.5e3f}, fb_stereo[2] = {22e3f, 54e3f};
    const float fb_rds[2] = {54e3f, 60e3f}, fb_rds_sq[2] = {113.5e3f, 114.5e3f};
    sdr_impulse_response_lpf((float)in.rf_Fs, 100000.0f, (unsigned short)T, rf.data());                  // rffrontend.cpp:24
    sdr_impulse_response_lpf_gain((float)(in.if_Fs * U), 16000.0f, (unsigned short)(T * U), U, audio.data()); // mono.cpp:22
    sdr_impulse_response_bpf((float)(in.rf_Fs / in.rf_decim), fb_pilot, (unsigned short)T, pilot.data());  // stereo.cpp:65
    sdr_impulse_response_bpf((float)(in.rf_Fs / in.rf_decim), fb_stereo, (unsigned short)T, stereo.data()); // stereo.cpp:67
    sdr_impulse_response_lpf_gain((float)(in.if_Fs * 247), 3e3f, (unsigned short)(T * 247), 247, rdsbb.data()); // rds.cpp:61
    sdr_impulse_response_bpf((float)in.if_Fs, fb_rds, (unsigned short)T, rds.data());                      // rds.cpp:62
    sdr_impulse_response_bpf((float)in.if_Fs, fb_rds_sq, (unsigned short)T, rds_sq.data());                // rds.cpp:63
    sdr_impulse_response_rrc((float)(2375 * in.symbol_Fs), (unsigned short)T, rrc.data());                 // rds.cpp:65
    Polyphase pa = make_polyphase(audio, U), pr = make_polyphase(rdsbb, 247);
    c->audio_L = pa.L;
    c->rdsbb_L = pr.L;
#define TRY(x) do { int r_ = (x); if (r_) { sdr_ctx_destroy(c); return r_; } } while (0)
    TRY(upload(c, &c->rf_h, rf));
    {
        // exact front-end tap table: row S (input sample S of a thread window, R outputs) holds
        // h[r*D + 100 - S] / 128 (exact power-of-two scaling) or 0 where that tap does not exist;
        // 32 zero floats past the last row (whole 128-byte tap batches are loaded)
        const int R = frontend_tab_r(), D = in.rf_decim, TWIN = (R - 1) * D + T;
        std::vector<float> tt((size_t)TWIN * R + 32, 0.0f);
        for (int S_ = 0; S_ < TWIN; S_++)
            for (int r = 0; r < R; r++) {
                const int k = r * D + (T - 1) - S_;
                if (k >= 0 && k < T) tt[(size_t)S_ * R + r] = rf[k] * 0.0078125f;
            }
        TRY(upload(c, &c->rf_hs, tt));
    }
    if (T == 101 && (in.rf_decim == 10 || in.rf_decim == 4 || in.rf_decim == 3)) {
        // tuned front end (sdr_frontend_tuned): the same table for its outputs per lane, and the
        // rotator's quarter table (the first quadrant's cosines of sdr_tuner_table); the tuning itself
        // comes with sdr_tuner_set
        const int R = frontend_tuned_r(), D = in.rf_decim, TWIN = (R - 1) * D + T;
        std::vector<float> tt((size_t)TWIN * R + 32, 0.0f);
        for (int S_ = 0; S_ < TWIN; S_++)
            for (int r = 0; r < R; r++) {
                const int k = r * D + (T - 1) - S_;
                if (k >= 0 && k < T) tt[(size_t)S_ * R + r] = rf[k] * 0.0078125f;
            }
        TRY(upload(c, &c->rf_ht, tt));
        const int N = frontend_tuned_n(D);
        std::vector<float> q((size_t)2 * N);
        int nt = 0;
        if (N != in.rf_Fs / 1000 || sdr_tuner_table(mode, q.data(), N, &nt) != SDR_OK || nt != N)
            TRY(fail(SDR_E_INVALID, "tuner: no rotator table for rf_Fs %d", in.rf_Fs));
        for (int k = 0; k <= N / 4; k++) q[(size_t)k] = q[(size_t)2 * k];   // cos(2 pi k / N)
        q.resize((size_t)N / 4 + 1);
        TRY(upload(c, &c->tn_q, q));
        TRY(dalloc(c, &c->tn_tab, (size_t)4 * nch));
        c->nxcc = device_xccs(device);
    }
    if (T == 101 && (in.rf_decim == 10 || in.rf_decim == 4 || in.rf_decim == 3)) {
        // MFMA front end: taps as fixed point h*2^F in FT_ND balanced base-256 digits, laid out as
        // the A fragments of v_mfma_i32_16x16x64_i8: fragment f = FT_ND*kstep + digit, lane l holds
        // A[row l&15][k = 64*kstep + 16*(l>>4) + jj], A[i][k] = digit(h[D*i + 100 - k])
        const int D = in.rf_decim;
        double hmax = 0.0;
        for (float v : rf) hmax = std::max(hmax, (double)std::fabs(v));
        const int F = 8 * FT_ND - 2 - (int)std::ceil(std::log2(hmax));   // |h * 2^F| < 2^(8*ND - 2)
        std::vector<int8_t> dig((size_t)T * FT_ND);
        for (int k = 0; k < T; k++) {
            long long q = std::llround((double)rf[k] * std::ldexp(1.0, F));
            for (int p = FT_ND - 1; p >= 0; p--) {               // least significant digit first
                int d = (int)(((q % 256) + 256) % 256);
                if (d >= 128) d -= 256;
                dig[(size_t)k * FT_ND + p] = (int8_t)d;
                q = (q - d) / 256;
            }
        }
        std::vector<int8_t> fr((size_t)FT_AFRAGS * 64 * 16, 0);
        for (int ks = 0; ks < 4; ks++)
            for (int p = 0; p < FT_ND; p++)
                for (int l = 0; l < 64; l++)
                    for (int jj = 0; jj < 16; jj++) {
                        const int i = l & 15, k = 64 * ks + 16 * (l >> 4) + jj, tap = D * i + 100 - k;
                        if (tap >= 0 && tap < T)
                            fr[(((size_t)(FT_ND * ks + p) * 64) + l) * 16 + jj] = dig[(size_t)tap * FT_ND + p];
                    }
        int8_t* dfr = nullptr;
        TRY(upload(c, &dfr, fr));
        c->fe_afrag = dfr;
        c->fe_yscale = std::ldexp(1.0, -(F + 7));
    }
    TRY(upload(c, &c->pilot_h, pilot));
    TRY(upload(c, &c->stereo_h, stereo));
    {
        // {pilot[k], band[k]} interleaved for the 3-filter pass's packed pairs, 104 pairs (chunks of 4)
        std::vector<float> h01(2 * 104, 0.0f);
        for (int k = 0; k < T && k < 104; k++) { h01[2 * k] = pilot[k]; h01[2 * k + 1] = stereo[k]; }
        TRY(upload(c, &c->pilot_band_h, h01));
    }
    TRY(upload(c, &c->rds_h, rds));
    TRY(upload(c, &c->rds_sq_h, rds_sq));
    TRY(upload(c, &c->rrc_h, rrc));
    TRY(upload(c, &c->audio_pp, pa.table));
    TRY(upload(c, &c->audio_cnt, pa.cnt));
    TRY(upload(c, &c->rdsbb_pp, pr.table));
    TRY(upload(c, &c->rdsbb_cnt, pr.cnt));
    c->rdsbb_all101 = std::all_of(pr.cnt.begin(), pr.cnt.end(), [](int k) { return k == 101; });
    c->audio_u1_101 = in.audio_upsample == 1 && pa.cnt.size() == 1 && pa.cnt[0] == 101;
    // ---- extended streams ----
    c->fm_stride = round_up((size_t)HIST + in.block_if, 64);
    c->rf_stride = round_up((size_t)HIST + in.n_rds, 64);
    c->fm_par = c->fm_stride * nch;
    c->rf_par = c->rf_stride * nch;
    float* base = nullptr;
    TRY(dalloc(c, &base, 2 * c->fm_par)); c->fm = base + HIST;
    TRY(dalloc(c, &base, 2 * c->fm_par)); c->sdc = base + HIST;
    TRY(dalloc(c, &base, 2 * c->fm_par)); c->rband = base + HIST;
    TRY(dalloc(c, &base, 2 * c->fm_par)); c->rdc = base + HIST;
    TRY(dalloc(c, &base, 2 * c->rf_par)); c->rfilt = base + HIST;
    if (flags & SDR_FLAG_RDS_QUAD) {
        TRY(dalloc(c, &base, 2 * c->fm_par)); c->rdc_q = base + HIST;
        TRY(dalloc(c, &base, 2 * c->rf_par)); c->rfilt_q = base + HIST;
    }
    if (flags & SDR_FLAG_IF_ENVELOPE) TRY(dalloc(c, &c->if_env, 2 * c->fm_par));
    c->plain_stride = round_up((size_t)in.block_if, 64);
    c->pll_stride = round_up((size_t)in.block_if + 1, 64);
    c->clean_stride = round_up((size_t)in.n_rds, 64);
    c->plain_par = c->plain_stride * nch;
    c->pll_par = c->pll_stride * nch;
    TRY(dalloc(c, &c->pilot, 2 * c->plain_par));
    TRY(dalloc(c, &c->band, 2 * c->plain_par));
    TRY(dalloc(c, &c->gpilot, 2 * c->plain_par));
    TRY(dalloc(c, &c->pilot_neg, 2 * c->plain_par));
    TRY(dalloc(c, &c->gpilot_neg, 2 * c->plain_par));
    TRY(dalloc(c, &c->t_st, 2 * c->plain_par));
    TRY(dalloc(c, &c->t_rds, 2 * c->plain_par));
    {
        std::vector<int> ptq(std::max(in.n_rds, 1));
        for (int k = 0; k < in.n_rds; k++) {                // rds.cpp:130: U = 247, D = 640
            const long long nd = (long long)k * 640;
            ptq[k] = (int)((nd / 247) << 8) | (int)(nd % 247);
        }
        TRY(upload(c, &c->rds_ptq, ptq));
    }
    TRY(dalloc(c, &c->rx_st, 2 * c->plain_par));
    TRY(dalloc(c, &c->rx_rds, 2 * c->plain_par));
    TRY(dalloc(c, &c->carrier, 2 * c->pll_par));
    TRY(dalloc(c, &c->ipll, 2 * c->pll_par));
    TRY(dalloc(c, &c->rds_clean, c->clean_stride * nch));
    if (flags & SDR_FLAG_RDS_QUAD) {
        TRY(dalloc(c, &c->rds_clean_q, c->clean_stride * nch));
        TRY(dalloc(c, &c->ipll_q_last, (size_t)2 * nch));
    }
    TRY(dalloc(c, &c->tail, (size_t)2 * nch * 2 * (T - 1)));
    {
        std::vector<uint32_t> pad(64, 0x80808080u);
        TRY(upload(c, &c->pad80, pad));
    }
    TRY(dalloc(c, &c->prev, (size_t)2 * nch));
    TRY(dalloc(c, &c->st_pll, (size_t)nch));
    TRY(dalloc(c, &c->rds_pll, (size_t)nch));
    TRY(dalloc(c, &c->dec, (size_t)nch * DEC_STATE));
    TRY(dalloc(c, &c->rel.words, (size_t)2 * sdr_ctx::Rel::SLOTS));
    TRY(dalloc(c, &c->rel.fail_words, (size_t)2));
    {
        // the release timeout's host-visible mirror: one coherent host word the device sets only on
        // the failure path, so that every stage call can check it without a synchronisation
        void* hp = nullptr;
        if (hipHostMalloc(&hp, 64, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess || !hp)
            TRY(fail(SDR_E_NOMEM, "hipHostMalloc of the context's fail word"));
        c->rel.fail_host = static_cast<uint32_t*>(hp);
        *c->rel.fail_host = 0u;
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess || !dp)
            TRY(fail(SDR_E_HIP, "hipHostGetDevicePointer of the context's fail word"));
        c->rel.fail_host_dev = static_cast<uint32_t*>(dp);
    }
    TRY(init_state(c, nullptr));
#undef TRY
    *out = c;
    return SDR_OK;
}

int sdr_ctx_destroy(sdr_ctx* c) {
    if (!c) return SDR_OK;
    (void)hipSetDevice(c->device);
    for (void* p : c->allocs) (void)hipFree(p);
    if (c->rel.fail_host) (void)hipHostFree(c->rel.fail_host);
    if (c->pers.ev) (void)hipEventDestroy(c->pers.ev);
    for (hipEvent_t e : c->fe_time.ev) (void)hipEventDestroy(e);
    if (c->fe_time.stamps) (void)hipFree(c->fe_time.stamps);
    for (hipEvent_t e : c->pers.reader_ev)
        if (e) (void)hipEventDestroy(e);
    delete c;
    return SDR_OK;
}

int sdr_ctx_reset(sdr_ctx* c, void* stream) {
    if (!c) return fail(SDR_E_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    c->pers.failed = false;   // a timed-out launch's poisoned state is what the reset replaces
    // no block of the reset context belongs to the last launch any more (its error word stays set
    // until the next launch's prepare: a block with the old index must not read it)
    c->pers.block = -1;
    c->pers.nreaders = 0;     // (the caller has drained its streams: nothing left to order after)
    // the release words back in step with the host's counts (a reader that never ran would leave its
    // slot short, and every later wait on it would expire again), then the release timeout cleared:
    // callers reset once the streams that ran the context's stages have drained
    hipStream_t s = S(stream);
    HIP_TRY(hipMemcpyAsync(c->rel.words, c->rel.seq, sizeof(c->rel.seq), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(c->rel.fail_words, 0, 2 * sizeof(uint32_t), s));
    const int r = init_state(c, s);   // (synchronises s)
    __atomic_store_n(c->rel.fail_host, 0u, __ATOMIC_SEQ_CST);
    return r;
}

int sdr_ctx_info(const sdr_ctx* c, sdr_info* info) {
    if (!c || !info) return fail(SDR_E_INVALID, "null argument");
    *info = c->info;
    return SDR_OK;
}

int sdr_ctx_buffer(sdr_ctx* c, const char* name, const float** ptr, size_t* stride, int* len) {
    if (!c || !name || !ptr || !stride || !len) return fail(SDR_E_INVALID, "null argument");
    const sdr_info& in = c->info;
    const int p = c->parity;
    if (std::strcmp(name, "if_env") == 0) {
        // SDR_FLAG_IF_ENVELOPE: the current block's IF power row, if a front end wrote one for it
        if (!c->if_env) return fail(SDR_E_INVALID, "buffer if_env needs SDR_FLAG_IF_ENVELOPE");
        if (c->block < 0 || c->env_block != c->block)
            return fail(SDR_E_INVALID, "buffer if_env: the current block has none (no front end yet, or sdr_push_fm_demod)");
        *ptr = c->if_env + p * c->fm_par;
        *stride = c->fm_stride;
        *len = in.block_if;
        return SDR_OK;
    }
    struct E { const char* n; const float* p; size_t s; int l; } tab[] = {
        {"fm", c->fm_cur(), c->fm_stride, in.block_if},
        {"pilot", c->plain(c->pilot), c->plain_stride, in.block_if},
        {"carrier", c->pllbuf(c->carrier), c->pll_stride, in.block_if + 1},
        {"band", c->plain(c->band), c->plain_stride, in.block_if},
        {"stereo_dc", c->sdc + p * c->fm_par, c->fm_stride, in.block_if},
        {"rds_band", c->rband + p * c->fm_par, c->fm_stride, in.block_if},
        {"gen_pilot", c->plain(c->gpilot), c->plain_stride, in.block_if},
        {"ipll", c->pllbuf(c->ipll), c->pll_stride, in.block_if + 1},
        {"rds_dc", c->rdc + p * c->fm_par, c->fm_stride, in.block_if},
        {"rds_filt", c->rfilt + p * c->rf_par, c->rf_stride, in.n_rds},
        {"rds_clean", c->rds_clean, c->clean_stride, in.n_rds},
        // SDR_FLAG_RDS_QUAD only (null pointers without it: refused below)
        {"rds_dc_q", c->rdc_q ? c->rdc_q + p * c->fm_par : nullptr, c->fm_stride, in.block_if},
        {"rds_filt_q", c->rfilt_q ? c->rfilt_q + p * c->rf_par : nullptr, c->rf_stride, in.n_rds},
        {"rds_clean_q", c->rds_clean_q, c->clean_stride, in.n_rds},
    };
    for (const E& e : tab) {
        if (std::strcmp(e.n, name) == 0) {
            if (!e.p) return fail(SDR_E_INVALID, "buffer %s needs SDR_FLAG_RDS_QUAD", name);
            *ptr = e.p;
            *stride = e.s;
            *len = e.l;
            return SDR_OK;
        }
    }
    return fail(SDR_E_INVALID, "unknown buffer %s", name);
}

int sdr_ctx_rds_clean_q(sdr_ctx* c, const float** ptr, size_t* stride, int* len) {
    return sdr_ctx_buffer(c, "rds_clean_q", ptr, stride, len);
}

}  // extern "C"
