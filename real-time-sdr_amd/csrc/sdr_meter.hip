// sdr_meter.hip -- reception meter on MI355X (gfx950): per channel and block, the readings a
// monitoring receiver shows (tuning offset, level, stereo pilot, RDS sub-carrier, noise, eye opening,
// audio peak and power), reduced from rows the pipeline already keeps in HBM, and the host-side
// arithmetic that turns a row into ratios and flags. No reference counterpart.
//
// Three kernels, one launch per call, one workgroup of 256 threads per channel:
//   k_meter_audio   fm (with its 100 history samples) is staged once in LDS and serves the fm sums and
//                   the noise FIR; the FIR (101 taps, every fifth output, the reference's convolveFIR
//                   order, filter.cpp:106-121) is fused with its square-and-sum, y is never stored;
//                   the pilot row and the int16 L/R row are read once from HBM.
//   k_meter_rds     the rds_band row is read once; rds_clean is staged in LDS for cdr()
//                   (rds_utilities.cpp:4-21) and the eye samples at the offset it returns.
//   k_meter_rf      the IF power row the front ends keep with SDR_FLAG_IF_ENVELOPE is read once: its sum,
//                   its sum of squares, its minimum and maximum, into a row array of its own.
//
// Summation order (a numpy model reproduces every float bit for bit; no FMA, each product and sum
// rounded on its own): a float sum over a row of length m has 256 partials, partial p adding the
// elements i = p, p + 256, ... in ascending i from +0 -- thread p's loop -- then eight pairing levels
// P[p] = P[p] + P[p + w], p < w, w = 128 .. 1: two through LDS, six as lane shifts inside wave 0. The
// eye sums have 64 partials (the lanes of wave 0) and the six lane-shift levels. Integer sums and
// every maximum are order-free.
//
// A channel's row is written by one workgroup with plain stores, each call its own fields; the flags
// word alone is shared by the two calls (which may run on two streams), so each ORs its bit in.
#include "stage_host.h"

#include <cmath>

#pragma clang fp contract(off)

namespace sdrk {
namespace {

constexpr int MT = 256;        // threads per workgroup = partials of a row sum
constexpr int NOISE_T = 101;   // taps of the noise band-pass
constexpr int NOISE_D = 5;     // every fifth output
constexpr int NOISE_H = NOISE_T - 1;

__device__ __forceinline__ int32_t cvt_i32_x86(float v) {   // (int)float of the reference's x86 build
    return (v >= -2147483648.0f && v < 2147483648.0f) ? (int32_t)v : INT32_MIN;
}

// the six pairing levels of 64 partials held by the lanes of one wave: lane 0 returns P[0]
// (lane p reads lane p + w, which the level before left valid for p + w < 2 w)
__device__ __forceinline__ float pair_wave(float v) {
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) v = v + __shfl_down(v, w, 64);
    return v;
}
// the eight pairing levels of NV sums of 256 partials, one partial of each per thread: thread 0 ends
// with every P[0] in v[]. red: [NV][MT] floats, free before the call (its barriers order what came before)
template <int NV>
__device__ __forceinline__ void pair_block(float (&v)[NV], float (*red)[MT]) {
    const int p = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NV; k++) red[k][p] = v[k];
    __syncthreads();
    if (p < 128) {
#pragma unroll
        for (int k = 0; k < NV; k++) red[k][p] = red[k][p] + red[k][p + 128];
    }
    __syncthreads();
    if (p < 64) {
#pragma unroll
        for (int k = 0; k < NV; k++) v[k] = pair_wave(red[k][p] + red[k][p + 64]);
    }
}
__device__ __forceinline__ float max_wave(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float min_wave(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ int max_wave(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ unsigned long long sum_wave(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

struct MeterAudio {
    const float* fm;        // this parity's fm_demod rows (data base: x[-HIST .. n) is readable)
    size_t fm_stride;
    const float* pilot;     // this parity's pilot rows
    size_t plain_stride;
    const float* h;         // NOISE_T taps
    const int16_t* lr;      // L/R interleaved rows, or null
    size_t lr_stride;
    int n, n_audio;
    sdr_meter_row* rows;
};

__global__ __launch_bounds__(MT) void k_meter_audio(const MeterAudio a) {
    extern __shared__ float xs[];          // x[-NOISE_H .. n) at xs[0 .. NOISE_H + n)
    __shared__ float red[4][MT];
    __shared__ float wpk[MT / 64];
    __shared__ int wip[2][MT / 64];
    __shared__ unsigned long long wsq[2][MT / 64];
    const int ch = blockIdx.x, p = threadIdx.x, wave = p >> 6;
    const int n = a.n;
    const float* __restrict__ x = a.fm + (size_t)ch * a.fm_stride;
    const float* __restrict__ pl = a.pilot + (size_t)ch * a.plain_stride;
    const float* __restrict__ h = a.h;

    if (p < NOISE_H) xs[p] = x[p - NOISE_H];
    float s = 0.0f, q = 0.0f, pk = 0.0f, pq = 0.0f;
    // both rows in one loop: twice the loads in flight
#pragma unroll 8
    for (int i = p; i < n; i += MT) {
        const float v = x[i], w = pl[i];
        xs[i + NOISE_H] = v;
        s = s + v;
        q = q + v * v;
        pk = fmaxf(pk, fabsf(v));   // (ignores NaN)
        pq = pq + w * w;
    }
    // audio: exact integers
    int lp = 0, rp = 0;
    unsigned long long lq = 0, rq = 0;
    if (a.lr) {
        const int16_t* __restrict__ lr = a.lr + (size_t)ch * a.lr_stride;
#pragma unroll 2
        for (int f = p; f < a.n_audio; f += MT) {
            const int l = lr[2 * f], r = lr[2 * f + 1];
            lp = max(lp, l < 0 ? -l : l);
            rp = max(rp, r < 0 ? -r : r);
            lq += (unsigned long long)(uint32_t)(l * l);
            rq += (unsigned long long)(uint32_t)(r * r);
        }
    }
    __syncthreads();
    // noise: y[j] = sum_k h[k] x[5 j - k] in ascending k from +0, then its square into partial j mod 256
    float nq = 0.0f;
    const int nj = n / NOISE_D;
    for (int j = p; j < nj; j += MT) {
        const float* w = xs + NOISE_D * j;   // w[NOISE_H - k] = x[5 j - k]
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < NOISE_T; k++) acc = acc + h[k] * w[NOISE_H - k];
        nq = nq + acc * acc;
    }

    float sums[4] = {s, q, pq, nq};
    pair_block(sums, red);
    pk = max_wave(pk);
    lp = max_wave(lp);
    rp = max_wave(rp);
    lq = sum_wave(lq);
    rq = sum_wave(rq);
    if ((p & 63) == 0) {
        wpk[wave] = pk;
        wip[0][wave] = lp;
        wip[1][wave] = rp;
        wsq[0][wave] = lq;
        wsq[1][wave] = rq;
    }
    __syncthreads();
    if (p == 0) {
        for (int w = 1; w < MT / 64; w++) {
            pk = fmaxf(pk, wpk[w]);
            lp = max(lp, wip[0][w]);
            rp = max(rp, wip[1][w]);
            lq += wsq[0][w];
            rq += wsq[1][w];
        }
        sdr_meter_row* row = a.rows + ch;
        row->fm_sum = sums[0];
        row->fm_sq = sums[1];
        row->fm_peak = pk;
        row->pilot_sq = sums[2];
        row->noise_sq = sums[3];
        row->l_peak = lp;
        row->r_peak = rp;
        row->l_sq = lq;
        row->r_sq = rq;
        __hip_atomic_fetch_or(&row->flags, SDR_METER_ROW_AUDIO, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct MeterRds {
    const float* rband;     // this parity's rds_band rows
    size_t fm_stride;
    const float* clean;     // the block's rds_clean rows
    size_t clean_stride;
    int n, n_rds, sps;
    sdr_meter_row* rows;
};

__global__ __launch_bounds__(MT) void k_meter_rds(const MeterRds a) {
    extern __shared__ float cs[];          // the channel's rds_clean row
    __shared__ float red[1][MT];
    const int ch = blockIdx.x, p = threadIdx.x;
    const float* __restrict__ rb = a.rband + (size_t)ch * a.fm_stride;
    const float* __restrict__ cl = a.clean + (size_t)ch * a.clean_stride;
    const int n_rds = a.n_rds, sps = a.sps;

    float rq[1] = {0.0f};
#pragma unroll 4
    for (int i = p; i < n_rds; i += MT) cs[i] = cl[i];
#pragma unroll 8
    for (int i = p; i < a.n; i += MT) {
        const float v = rb[i];
        rq[0] = rq[0] + v * v;
    }
    pair_block(rq, red);   // (its barriers also publish cs)
    if (p >= 64) return;

    // cdr(): argmax over offsets i < sps of sum_k |(int)x[k sps + i]|, the first maximum, 0 when
    // every sum is 0; one lane per offset, the argmax as a wave maximum of (sum, ~offset)
    const int nk = n_rds / sps;
    unsigned long long key = 0;
    for (int i = p; i < sps; i += 64) {
        uint32_t sum = 0;
        for (int k = 0; k < nk; k++) {
            const int32_t v = cvt_i32_x86(cs[k * sps + i]);
            sum += v < 0 ? -(uint32_t)v : (uint32_t)v;
        }
        const int32_t si = (int32_t)sum;
        const unsigned long long ki = si > 0 ? ((unsigned long long)(uint32_t)si << 32) | (uint32_t)~(uint32_t)i : 0ull;
        if (ki > key) key = ki;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(key, m, 64);
        if (o > key) key = o;
    }
    const int off = key ? (int)~(uint32_t)(key & 0xFFFFFFFFull) : 0;
    // the eye: |rds_clean| at the symbol instants off + k sps < n_rds
    const int ne = off < n_rds ? (n_rds - off + sps - 1) / sps : 0;
    float ea = 0.0f, eq = 0.0f;
    for (int k = p; k < ne; k += 64) {
        const float v = fabsf(cs[off + k * sps]);
        ea = ea + v;
        eq = eq + v * v;
    }
    ea = pair_wave(ea);
    eq = pair_wave(eq);
    if (p == 0) {
        sdr_meter_row* row = a.rows + ch;
        row->rds_sq = rq[0];
        row->eye_abs = ea;
        row->eye_sq = eq;
        row->eye_n = ne;
        __hip_atomic_fetch_or(&row->flags, SDR_METER_ROW_RDS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct MeterRf {
    const float* env;       // this parity's if_env rows
    size_t stride;
    int n;
    sdr_meter_rf_row* rows;
};

// A row of its own per channel, written whole by thread 0 with plain stores: no word shared with the
// other two calls.
__global__ __launch_bounds__(MT) void k_meter_rf(const MeterRf a) {
    __shared__ float red[2][MT];
    __shared__ float wmn[MT / 64], wmx[MT / 64];
    const int ch = blockIdx.x, p = threadIdx.x, wave = p >> 6;
    const float* __restrict__ e = a.env + (size_t)ch * a.stride;
    float s = 0.0f, q = 0.0f, mx = 0.0f, mn = __builtin_inff();
#pragma unroll 8
    for (int i = p; i < a.n; i += MT) {
        const float v = e[i];
        s = s + v;
        q = q + v * v;
        mx = fmaxf(mx, v);          // (both ignore NaN)
        mn = fminf(mn, v);
    }
    float sums[2] = {s, q};
    pair_block(sums, red);
    mx = max_wave(mx);
    mn = min_wave(mn);
    if ((p & 63) == 0) {
        wmx[wave] = mx;
        wmn[wave] = mn;
    }
    __syncthreads();
    if (p == 0) {
        for (int w = 1; w < MT / 64; w++) {
            mx = fmaxf(mx, wmx[w]);
            mn = fminf(mn, wmn[w]);
        }
        sdr_meter_rf_row* row = a.rows + ch;
        row->env_sum = sums[0];
        row->env_sq = sums[1];
        row->env_min = mn;
        row->env_max = mx;
        row->n = a.n;
        row->flags = SDR_METER_ROW_RF;
        row->reserved[0] = row->reserved[1] = 0;
    }
}

// num / den of two mean powers: 0 for a zero numerator, +inf for a zero denominator under a positive one
double ratio(double num, double den) {
    if (!(num != 0.0)) return 0.0;
    if (den <= 0.0) return num > 0.0 ? HUGE_VAL : 0.0;
    return num / den;
}

}  // namespace
}  // namespace sdrk

using namespace sdrk;

extern "C" {

int sdr_meter_taps(int mode, float* h, int max, int* n) {
    sdr_info in;
    if (const int r = mode_info(&in, 1, mode, 1)) return r;
    if (n) *n = NOISE_T;
    if (!h) return n ? SDR_OK : fail(SDR_E_INVALID, "meter_taps: null argument");
    if (max < NOISE_T) return fail(SDR_E_INVALID, "meter_taps: room for %d of %d taps", max, NOISE_T);
    const float fb[2] = {75e3f, 84e3f};   // between the 67 kHz and 92 kHz SCA sub-carriers
    return sdr_impulse_response_bpf((float)in.if_Fs, fb, NOISE_T, h);
}

void sdr_meter_opts_default(sdr_meter_opts* o) {
    if (!o) return;
    o->pilot_nr_min = 1.0f;
    o->rds_nr_min = 4.0f;
    o->offtune_min = 0.25f;
    o->silence_peak = 64;
}

int sdr_meter_status(int mode, const sdr_meter_row* row, const sdr_meter_opts* o, sdr_meter_state* out) {
    sdr_info in;
    if (const int r = mode_info(&in, 1, mode, 1)) return r;
    if (!row || !o || !out) return fail(SDR_E_INVALID, "meter_status: null argument");
    const double n = in.block_if, n5 = in.block_if / NOISE_D;
    const double noise = (double)row->noise_sq / n5;
    out->offset = (double)row->fm_sum / n;
    out->level_db = 10.0 * std::log10((double)row->fm_sq / n);
    out->pilot_nr = ratio((double)row->pilot_sq / n, noise);
    out->rds_nr = ratio((double)row->rds_sq / n, noise);
    double eye = 0.0;
    if (row->eye_n > 0) {
        const double m1 = (double)row->eye_abs / row->eye_n, m2 = (double)row->eye_sq / row->eye_n;
        eye = ratio(m1 * m1, m2 - m1 * m1);
    }
    out->eye_db = 10.0 * std::log10(eye);
    int f = 0;
    if (out->pilot_nr >= (double)o->pilot_nr_min) f |= SDR_METER_STEREO;
    if (out->rds_nr >= (double)o->rds_nr_min) f |= SDR_METER_RDS;
    if (std::fabs(out->offset) >= (double)o->offtune_min) f |= SDR_METER_OFFTUNE;
    if ((row->flags & SDR_METER_ROW_AUDIO) && row->l_peak <= o->silence_peak && row->r_peak <= o->silence_peak)
        f |= SDR_METER_DEAD_AIR;
    out->flags = f;
    return SDR_OK;
}

void sdr_meter_rf_opts_default(sdr_meter_rf_opts* o) {
    if (!o) return;
    o->ripple_max = 21.0f / 121.0f;
}

int sdr_meter_rf_status(int mode, const sdr_meter_rf_row* row, const sdr_meter_rf_opts* o, sdr_meter_rf_state* out) {
    sdr_info in;
    if (const int r = mode_info(&in, 1, mode, 1)) return r;
    if (!row || !o || !out) return fail(SDR_E_INVALID, "meter_rf_status: null argument");
    const double n = row->n;
    const double m1 = row->n > 0 ? (double)row->env_sum / n : 0.0, m2 = row->n > 0 ? (double)row->env_sq / n : 0.0;
    const bool zero = !(m1 != 0.0);
    out->level_dbfs = 10.0 * std::log10(m1);
    out->ripple = zero ? 0.0 : (m2 - m1 * m1) / (m1 * m1);
    const double S = std::sqrt(std::max(2.0 * m1 * m1 - m2, 0.0)), N = m1 - S;
    if (!(S > 0.0)) out->cnr_db = -HUGE_VAL;
    else if (N <= 0.0) out->cnr_db = HUGE_VAL;
    else out->cnr_db = 10.0 * std::log10(S / N);
    out->fade_db = zero ? 0.0 : 10.0 * std::log10((double)row->env_min / m1);
    out->crest_db = zero ? 0.0 : 10.0 * std::log10((double)row->env_max / m1);
    int f = 0;
    if ((row->flags & SDR_METER_ROW_RF) && (zero || out->ripple > (double)o->ripple_max)) f |= SDR_METER_RF_WEAK;
    out->flags = f;
    return SDR_OK;
}

int sdr_meter_deviation(int mode, const sdr_meter_row* row, double* peak_khz, double* rms_khz, double* offset_khz) {
    sdr_info in;
    if (const int r = mode_info(&in, 1, mode, 1)) return r;
    if (!row) return fail(SDR_E_INVALID, "meter_deviation: null row");
    const double n = in.block_if, k = (double)in.if_Fs / (2.0 * 3.14159265358979323846) / 1000.0;
    if (peak_khz) *peak_khz = (double)row->fm_peak * k;
    if (rms_khz) *rms_khz = std::sqrt((double)row->fm_sq / n) * k;
    if (offset_khz) *offset_khz = (double)row->fm_sum / n * k;
    return SDR_OK;
}

int sdr_meter_create(sdr_meter** out, int device, int nch, int mode) {
    if (!out) return fail(SDR_E_INVALID, "meter_create: out is NULL");
    *out = nullptr;
    sdr_info in;
    if (const int r = mode_info(&in, nch, mode, 1)) return r;
    if (nch < 1) return fail(SDR_E_INVALID, "meter_create: nch %d < 1", nch);
    float h[NOISE_T];
    int nt = 0;
    if (const int r = sdr_meter_taps(mode, h, NOISE_T, &nt)) return r;
    sdr_meter* m = nullptr;
    if (const int r = create_begin(&m, device, "meter_create")) return r;
    m->nch = nch;
    m->mode = mode;
    hipError_t e = hipSuccess;
    dev_alloc(e, &m->h, sizeof(h));
    dev_alloc(e, &m->rows, (size_t)nch * sizeof(sdr_meter_row));
    dev_alloc(e, &m->rf_rows, (size_t)nch * sizeof(sdr_meter_rf_row));
    if (e == hipSuccess) e = hipMemcpy(m->h, h, sizeof(h), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(m->rows, 0, (size_t)nch * sizeof(sdr_meter_row));
    if (e == hipSuccess) e = hipMemset(m->rf_rows, 0, (size_t)nch * sizeof(sdr_meter_rf_row));
    return create_done(e, m, out, sdr_meter_destroy, "meter_create");
}

int sdr_meter_destroy(sdr_meter* m) {
    if (!m) return fail(SDR_E_INVALID, "meter_destroy: null meter");
    return destroy_handle(m, {m->h, m->rows, m->rf_rows});
}

int sdr_meter_reset(sdr_meter* m, void* stream) {
    if (!m) return fail(SDR_E_INVALID, "meter_reset: null meter");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemsetAsync(m->rows, 0, (size_t)m->nch * sizeof(sdr_meter_row), (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(m->rf_rows, 0, (size_t)m->nch * sizeof(sdr_meter_rf_row), (hipStream_t)stream));
    return SDR_OK;
}

// the checks the calls share: handles, the context's state, the same shape and device
static int meter_check(const sdr_meter* m, const sdr_ctx* c, const char* what) {
    if (!m || !c) return fail(SDR_E_INVALID, "%s: null handle", what);
    if (const int rf = check_failed(c, what)) return rf;
    if (c->nch != m->nch || c->mode != m->mode || c->device != m->device)
        return fail(SDR_E_INVALID, "%s: the context (nch %d, mode %d, device %d) is not the meter's (%d, %d, %d)", what,
                    c->nch, c->mode, c->device, m->nch, m->mode, m->device);
    return SDR_OK;
}

int sdr_meter_audio(sdr_meter* m, sdr_ctx* c, const int16_t* lr, size_t lr_stride, void* stream) {
    if (const int r = meter_check(m, c, "meter_audio")) return r;
    const sdr_info& in = c->info;
    if (c->block < 0 || c->st_pre_done != c->block)
        return fail(SDR_E_INVALID, "meter_audio: run sdr_stereo_pre (or sdr_pre) on the current block first");
    if (lr && lr_stride < (size_t)2 * in.n_audio)
        return fail(SDR_E_INVALID, "meter_audio: lr_stride %zu < 2*n_audio %d", lr_stride, 2 * in.n_audio);
    HIP_TRY(hipSetDevice(m->device));
    MeterAudio a{};
    a.fm = c->fm_cur();
    a.fm_stride = c->fm_stride;
    a.pilot = c->plain(c->pilot);
    a.plain_stride = c->plain_stride;
    a.h = m->h;
    a.lr = lr;
    a.lr_stride = lr_stride;
    a.n = in.block_if;
    a.n_audio = in.n_audio;
    a.rows = m->rows;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_meter_audio, dim3(m->nch), dim3(MT), (size_t)(NOISE_H + in.block_if) * sizeof(float), s, a);
    LAUNCH_CHECK();
    return release_record(c, REL_METER_A, s);   // fm and pilot of this parity read
}

int sdr_meter_rds(sdr_meter* m, sdr_ctx* c, void* stream) {
    if (const int r = meter_check(m, c, "meter_rds")) return r;
    const sdr_info& in = c->info;
    if (!c->rds_on) return fail(SDR_E_INVALID, "meter_rds: the context has no RDS chain (rds_on = 0)");
    if (c->block < 0 || c->rds_pre_done != c->block || c->rds_dsp_done != c->block)
        return fail(SDR_E_INVALID, "meter_rds: run sdr_rds_pre and sdr_rds_post (or sdr_rds_dsp) on the current block first");
    HIP_TRY(hipSetDevice(m->device));
    MeterRds a{};
    a.rband = c->rband + c->parity * c->fm_par;
    a.fm_stride = c->fm_stride;
    a.clean = c->rds_clean;
    a.clean_stride = c->clean_stride;
    a.n = in.block_if;
    a.n_rds = in.n_rds;
    a.sps = in.symbol_Fs;
    a.rows = m->rows;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_meter_rds, dim3(m->nch), dim3(MT), (size_t)in.n_rds * sizeof(float), s, a);
    LAUNCH_CHECK();
    return release_record(c, REL_METER_R, s);   // rds_band of this parity read
}

int sdr_meter_rf(sdr_meter* m, sdr_ctx* c, void* stream) {
    if (const int r = meter_check(m, c, "meter_rf")) return r;
    if (!c->if_env) return fail(SDR_E_INVALID, "meter_rf: the context has no IF envelope row (SDR_FLAG_IF_ENVELOPE)");
    if (c->block < 0 || c->env_block != c->block)
        return fail(SDR_E_INVALID, "meter_rf: the current block has no IF envelope row (no front end yet, or "
                                   "sdr_push_fm_demod brought it)");
    HIP_TRY(hipSetDevice(m->device));
    MeterRf a{};
    a.env = c->if_env + c->parity * c->fm_par;
    a.stride = c->fm_stride;
    a.n = c->info.block_if;
    a.rows = m->rf_rows;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_meter_rf, dim3(m->nch), dim3(MT), 0, s, a);
    LAUNCH_CHECK();
    return release_record(c, REL_METER_RF, s);   // if_env of this parity read
}

int sdr_meter_rf_read(sdr_meter* m, sdr_meter_rf_row* host_rows, void* stream) {
    if (!m || !host_rows) return fail(SDR_E_INVALID, "meter_rf_read: null argument");
    HIP_TRY(hipSetDevice(m->device));
    return copy_records(m->rf_rows, host_rows, m->nch, S(stream));
}

int sdr_meter_rf_rows(sdr_meter* m, const sdr_meter_rf_row** dev) {
    if (!m || !dev) return fail(SDR_E_INVALID, "meter_rf_rows: null argument");
    *dev = m->rf_rows;
    return SDR_OK;
}

int sdr_meter_read(sdr_meter* m, sdr_meter_row* host_rows, void* stream) {
    if (!m || !host_rows) return fail(SDR_E_INVALID, "meter_read: null argument");
    HIP_TRY(hipSetDevice(m->device));
    return copy_records(m->rows, host_rows, m->nch, S(stream));
}

int sdr_meter_rows(sdr_meter* m, const sdr_meter_row** dev) {
    if (!m || !dev) return fail(SDR_E_INVALID, "meter_rows: null argument");
    *dev = m->rows;
    return SDR_OK;
}

}  // extern "C"
