// sdr_audio.hip -- audio finishing on MI355X (gfx950): de-emphasis (a one-pole per audio channel), a
// stereo blend driven by the reception meter's pilot reading, and a gain with click-free ramps, over
// the int16 rows the stereo or mono stage wrote. No reference counterpart; the definition is in
// include/sdr_amd.h (sdr_audio_*) and a numpy model (tests/audio_model.py) reproduces every bit.
//
// k_audio_finish, one launch per call. Only y <- fl(fl(a y) + c[n]) is serial: nch * width chains of
// N steps, two dependent f32 operations a step. A workgroup of five waves owns CG channels and walks
// their rows in tiles of T frames through a ring of three LDS buffers [chain][T + 1] (the odd row
// length keeps a wave's column reads on 32 different banks):
//   waves 1-4  load the int16 rows of tile i + 1 into registers (coalesced along the rows), turn the
//              registers of tile i into c[n] = fl(b x[n]) -- blend and ramps included -- in buffer
//              i mod 3, and turn the y of tile i - 2 into int16 (gain, rounding, clamp) and store it
//   wave 0     one lane per chain, runs tile i - 1 in place (c[n] read eight steps ahead, y[n] written
//              over it)
// with one barrier per tile; the chain never waits for global memory.
// k_audio_blend, k_audio_control and k_audio_reset write the small per-channel state.
#include "stage_host.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#pragma clang fp contract(off)

struct sdr_audio {
    int device = 0, nch = 0, mode = 0, width = 0, n = 0, block_if = 0, shape = 0;
    float a = 0.0f, b = 1.0f, lo = 0.0f, hi = 0.0f;
    sdr_audio_state* st = nullptr;   // [nch] (device)
    float* ctl = nullptr;            // [2][nch] pinned: the targets sdr_audio_set_control hands to its kernel
    hipEvent_t ctl_read = nullptr;   // that kernel has read them
};

namespace sdrk {
namespace {

constexpr int AW = 256;          // worker threads (waves 1-4)
constexpr int ANT = AW + 64;     // wave 0 runs the chains
constexpr int AU = 8;            // steps the chain wave reads ahead

struct AudioFinish {
    const int16_t* in;
    size_t in_stride;
    int16_t* out;
    size_t out_stride;
    sdr_audio_state* st;
    int nch, n;
    float a, b, rn;
};

template <int W>
using frame_t = std::conditional_t<W == 2, uint32_t, uint16_t>;   // one frame of a row
template <int W>
constexpr frame_t<W> POISON_FRAME = (frame_t<W>)((uint32_t)(uint16_t)SDR_PCM_POISON * (W == 2 ? 0x10001u : 1u));

__device__ __forceinline__ uint16_t finish_i16(float v, float y) {
    const float r = rintf(v * y);
    return (uint16_t)(int16_t)fminf(fmaxf(r, -32767.0f), 32767.0f);
}

// tl steps of one chain over its tile, in place: p[n] = c[n] in, y[n] out
template <int T>
__device__ __forceinline__ float chain_tile(float* p, int tl, float a, float y) {
    if (tl == T) {
        float cn[AU];
#pragma unroll
        for (int u = 0; u < AU; u++) cn[u] = p[u];
        for (int n = 0; n < T; n += AU) {
            float cc[AU];
#pragma unroll
            for (int u = 0; u < AU; u++) cc[u] = cn[u];
            if (n + AU < T) {
#pragma unroll
                for (int u = 0; u < AU; u++) cn[u] = p[n + AU + u];
            }
#pragma unroll
            for (int u = 0; u < AU; u++) {
                y = a * y + cc[u];
                p[n + u] = y;
            }
        }
    } else {
        for (int n = 0; n < tl; n++) {
            y = a * y + p[n];
            p[n] = y;
        }
    }
    return y;
}

template <int W, int CG, int T>
__global__ __launch_bounds__(ANT) void k_audio_finish(const AudioFinish q) {
    static_assert(T <= AW && AW % T == 0 && (CG * T) % AW == 0 && T % AU == 0 && CG * W <= 64, "shape");
    constexpr int CHAINS = CG * W, CPP = AW / T, K = CG / CPP;   // channels per pass of the workers, passes
    __shared__ float buf[3][CHAINS][T + 1];
    __shared__ float4 ramp[CG];      // g0, dg, v0, dv
    __shared__ int pois[CG];
    using F = frame_t<W>;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int ch0 = blockIdx.x * CG, N = q.n;
    const int ncg = min(CG, q.nch - ch0);
    const int ntiles = (N + T - 1) / T;

    // a poisoned row: every frame the poison pattern. The first frame decides for nearly every row and
    // thread c reads channel c's (one round trip for the group, not one per channel); only a row that
    // starts with the pattern is read through, by all threads
    if (tid < ncg) {
        const sdr_audio_state s = q.st[ch0 + tid];
        ramp[tid] = make_float4(s.blend, s.blend_target - s.blend, s.gain, s.gain_target - s.gain);
        pois[tid] = *reinterpret_cast<const F*>(q.in + (size_t)(ch0 + tid) * q.in_stride) == POISON_FRAME<W>;
    }
    __syncthreads();
    for (int c = 0; c < ncg; c++) {
        if (pois[c]) {                   // (the same for every thread)
            const F* row = reinterpret_cast<const F*>(q.in + (size_t)(ch0 + c) * q.in_stride);
            int ok = 1;
            for (int i = tid; i < N; i += ANT) ok &= row[i] == POISON_FRAME<W>;
            const int all = __syncthreads_and(ok);
            if (tid == 0) pois[c] = all;
        }
    }
    __syncthreads();

    // workers: thread wt handles frame f of channels k CPP + cl, k < K
    const int wt = tid - 64, f = wt & (T - 1), cl = wt / T;
    F cur[K] = {}, nxt[K] = {};
    auto load_tile = [&](int tile, F (&r)[K]) {
        const int n = tile * T + f;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int c = k * CPP + cl;
            r[k] = 0;
            if (c < ncg && n < N) r[k] = reinterpret_cast<const F*>(q.in + (size_t)(ch0 + c) * q.in_stride)[n];
        }
    };
    float y = 0.0f;                  // wave 0: lane's chain
    const int my_c = tid / W;        // wave 0: lane's channel in the group
    const bool chain_on = wave == 0 && tid < CHAINS && my_c < ncg;
    if (chain_on) y = q.st[ch0 + my_c].y[tid % W];
    if (wave == 0) __builtin_amdgcn_s_setprio(3);
    else load_tile(0, cur);

    // iteration `it`: the workers load tile it + 1, turn tile it into c[n] and store tile it - 2; the
    // chain wave runs tile it - 1
    for (int it = 0; it < ntiles + 2; it++) {
        if (wave == 0) {
            const int j = it - 1;
            if (chain_on && j >= 0 && j < ntiles) y = chain_tile<T>(&buf[j % 3][tid][0], min(T, N - j * T), q.a, y);
        } else {
            if (it + 1 < ntiles) load_tile(it + 1, nxt);
            if (it < ntiles) {
                const int n = it * T + f;
                const float t = (float)(n + 1) * q.rn;
                float(*c_out)[T + 1] = buf[it % 3];
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const int c = k * CPP + cl;
                    if (c < ncg && n < N) {
                        if (W == 2) {
                            const float4 rp = ramp[c];
                            const float g = rp.x + rp.y * t;
                            const float l = (float)(int16_t)(cur[k] & 0xFFFFu), r = (float)(int16_t)((uint32_t)cur[k] >> 16);
                            const float m = 0.5f * (l + r), s = 0.5f * (l - r);
                            const float p = g * s;
                            c_out[2 * c][f] = q.b * (m + p);
                            c_out[2 * c + 1][f] = q.b * (m - p);
                        } else {
                            c_out[c][f] = q.b * (float)(int16_t)cur[k];
                        }
                    }
                }
            }
            if (it >= 2) {
                const int n = (it - 2) * T + f;
                const float t = (float)(n + 1) * q.rn;
                const float(*y_in)[T + 1] = buf[(it - 2) % 3];
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const int c = k * CPP + cl;
                    if (c < ncg && n < N) {
                        const float4 rp = ramp[c];
                        const float v = rp.z + rp.w * t;
                        F* o = reinterpret_cast<F*>(q.out + (size_t)(ch0 + c) * q.out_stride) + n;
                        if (pois[c]) *o = POISON_FRAME<W>;
                        else if (W == 2)
                            *o = (F)((uint32_t)finish_i16(v, y_in[2 * c][f]) | ((uint32_t)finish_i16(v, y_in[2 * c + 1][f]) << 16));
                        else *o = (F)finish_i16(v, y_in[c][f]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < K; k++) cur[k] = nxt[k];
        }
        __syncthreads();
    }

    if (chain_on) q.st[ch0 + my_c].y[tid % W] = pois[my_c] ? 0.0f : y;
    if (wave == 1 && wt < ncg) {     // the ramps have arrived
        sdr_audio_state* s = q.st + ch0 + wt;
        s->blend = s->blend_target;
        s->gain = s->gain_target;
    }
}

__global__ __launch_bounds__(256) void k_audio_blend(const sdr_meter_row* __restrict__ rows, sdr_audio_state* st, int nch,
                                                     float n, float n5, float lo, float span) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nch) return;
    const sdr_meter_row r = rows[i];
    if (!(r.flags & SDR_METER_ROW_AUDIO)) return;
    const float P = r.pilot_sq * n5, Z = r.noise_sq * n;
    float g;
    if (!(P > 0.0f)) g = 0.0f;
    else if (Z == 0.0f) g = 1.0f;
    else {
        const float x = (P / Z - lo) / span;
        g = !(x > 0.0f) ? 0.0f : (x > 1.0f ? 1.0f : x);   // (NaN: 0)
    }
    st[i].blend_target = g;
}

__global__ __launch_bounds__(256) void k_audio_control(sdr_audio_state* st, int nch, const float* blend, const float* gain) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nch) return;
    if (blend) st[i].blend_target = blend[i];
    if (gain) st[i].gain_target = gain[i];
}

__global__ __launch_bounds__(256) void k_audio_reset(sdr_audio_state* st, int nch) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nch) return;
    st[i] = sdr_audio_state{{0.0f, 0.0f}, 1.0f, 1.0f, 1.0f, 1.0f};
}

// the shapes measured (tools/bench_audio.py): channels per workgroup, frames per tile
constexpr int SHAPES = 4;
template <int W>
void launch_finish(int shape, int nch, hipStream_t s, const AudioFinish& q) {
    switch (shape) {
    case 0: hipLaunchKernelGGL((k_audio_finish<W, 32, 64>), dim3((nch + 31) / 32), dim3(ANT), 0, s, q); break;
    case 1: hipLaunchKernelGGL((k_audio_finish<W, 16, 128>), dim3((nch + 15) / 16), dim3(ANT), 0, s, q); break;
    case 2: hipLaunchKernelGGL((k_audio_finish<W, 8, 128>), dim3((nch + 7) / 8), dim3(ANT), 0, s, q); break;
    default: hipLaunchKernelGGL((k_audio_finish<W, 4, 128>), dim3((nch + 3) / 4), dim3(ANT), 0, s, q); break;
    }
}

int coeffs(const sdr_info& in, float tau_us, float* a, float* b) {
    if (!(tau_us >= 0.0f) || !(tau_us <= 1000.0f))
        return fail(SDR_E_INVALID, "audio: tau_us %g is not in [0, 1000]", (double)tau_us);
    float fa = 0.0f;
    if (tau_us > 0.0f) {
        const double fs = (double)in.if_Fs * in.audio_upsample / in.audio_decim;
        fa = (float)std::exp(-1e6 / ((double)tau_us * fs));
    }
    *a = fa;
    *b = (float)(1.0 - (double)fa);
    return SDR_OK;
}

}  // namespace
}  // namespace sdrk

using namespace sdrk;

extern "C" {

void sdr_audio_opts_default(sdr_audio_opts* o) {
    if (!o) return;
    o->tau_us = 75.0f;
    o->blend_lo = 0.5f;
    o->blend_hi = 2.0f;
}

int sdr_audio_coeffs(int mode, float tau_us, float* a, float* b) {
    sdr_info in;
    if (const int r = mode_info(&in, 1, mode, 1)) return r;
    if (!a || !b) return fail(SDR_E_INVALID, "audio_coeffs: null argument");
    return coeffs(in, tau_us, a, b);
}

// the stage's rule for an options record in a mode (in); `who` names the caller in the text
static int audio_opts_rule(const char* who, const sdr_info& in, const sdr_audio_opts* o, float* a, float* b) {
    if (const int r = coeffs(in, o->tau_us, a, b)) return r;
    if (!std::isfinite(o->blend_lo) || !std::isfinite(o->blend_hi) || !(o->blend_hi > o->blend_lo))
        return fail(SDR_E_INVALID, "%s: blend_hi %g <= blend_lo %g", who, (double)o->blend_hi, (double)o->blend_lo);
    return SDR_OK;
}

int sdr_audio_opts_check(int mode, const sdr_audio_opts* o) {
    sdr_info in;
    if (const int r = mode_info(&in, 1, mode, 1)) return r;
    if (!o) return fail(SDR_E_INVALID, "audio_opts_check: opts is NULL");
    float a = 0.0f, b = 1.0f;
    return audio_opts_rule("audio_opts_check", in, o, &a, &b);
}

int sdr_audio_create(sdr_audio** out, int device, int nch, int mode, int width, const sdr_audio_opts* o) {
    if (!out) return fail(SDR_E_INVALID, "audio_create: out is NULL");
    *out = nullptr;
    if (!o) return fail(SDR_E_INVALID, "audio_create: opts is NULL");
    sdr_info in;
    if (const int r = mode_info(&in, nch, mode, 1)) return r;
    if (nch < 1) return fail(SDR_E_INVALID, "audio_create: nch %d < 1", nch);
    if (width != 1 && width != 2) return fail(SDR_E_INVALID, "audio_create: width %d is not 1 or 2", width);
    float ca = 0.0f, cb = 1.0f;
    if (const int r = audio_opts_rule("audio_create", in, o, &ca, &cb)) return r;
    int shape = 2;   // 8 channels per workgroup (4 measured 9 % faster alone: DESIGN 4e)
    if (const char* e = std::getenv("SDR_AUDIO_SHAPE")) {   // for A/B (tools/bench_audio.py)
        shape = std::atoi(e);
        if (shape < 0 || shape >= SHAPES) return fail(SDR_E_INVALID, "audio_create: SDR_AUDIO_SHAPE %s", e);
    }
    sdr_audio* a = nullptr;
    if (const int r = create_begin(&a, device, "audio_create")) return r;
    a->nch = nch;
    a->mode = mode;
    a->width = width;
    a->n = in.n_audio;
    a->block_if = in.block_if;
    a->shape = shape;
    a->a = ca;
    a->b = cb;
    a->lo = o->blend_lo;
    a->hi = o->blend_hi;
    hipError_t e = hipSuccess;
    dev_alloc(e, &a->st, (size_t)nch * sizeof(sdr_audio_state));
    if (e == hipSuccess) e = hipHostMalloc((void**)&a->ctl, (size_t)2 * nch * sizeof(float), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&a->ctl_read, hipEventDisableTiming);
    create_reset(e, k_audio_reset, groups256(nch), a->st, nch);
    return create_done(e, a, out, sdr_audio_destroy, "audio_create");
}

int sdr_audio_destroy(sdr_audio* a) {
    if (!a) return fail(SDR_E_INVALID, "audio_destroy: null handle");
    (void)hipSetDevice(a->device);
    (void)hipDeviceSynchronize();   // a pending call may still use the state
    if (a->st) (void)hipFree(a->st);
    if (a->ctl) (void)hipHostFree(a->ctl);
    if (a->ctl_read) (void)hipEventDestroy(a->ctl_read);
    delete a;
    return SDR_OK;
}

int sdr_audio_reset(sdr_audio* a, void* stream) {
    if (!a) return fail(SDR_E_INVALID, "audio_reset: null handle");
    return launch_on(a->device, k_audio_reset, groups256(a->nch), S(stream), a->st, a->nch);
}

int sdr_audio_set_control(sdr_audio* a, const float* blend, const float* gain, void* stream) {
    if (!a) return fail(SDR_E_INVALID, "audio_set_control: null handle");
    for (int i = 0; i < a->nch; i++) {
        if (blend && !(blend[i] >= 0.0f && blend[i] <= 1.0f))
            return fail(SDR_E_INVALID, "audio_set_control: blend[%d] = %g is not in [0, 1]", i, (double)blend[i]);
        if (gain && !(gain[i] >= 0.0f && std::isfinite(gain[i])))
            return fail(SDR_E_INVALID, "audio_set_control: gain[%d] = %g is negative or not finite", i, (double)gain[i]);
    }
    if (!blend && !gain) return SDR_OK;
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipEventSynchronize(a->ctl_read));   // the call before this one has read the pinned targets
    float* hb = a->ctl;
    float* hg = a->ctl + a->nch;
    if (blend) std::memcpy(hb, blend, (size_t)a->nch * sizeof(float));
    if (gain) std::memcpy(hg, gain, (size_t)a->nch * sizeof(float));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_audio_control, dim3((a->nch + 255) / 256), dim3(256), 0, s, a->st, a->nch,
                       blend ? (const float*)hb : nullptr, gain ? (const float*)hg : nullptr);
    LAUNCH_CHECK();
    HIP_TRY(hipEventRecord(a->ctl_read, s));
    return SDR_OK;
}

int sdr_audio_blend_from_meter(sdr_audio* a, sdr_meter* m, void* stream) {
    if (!a || !m) return fail(SDR_E_INVALID, "audio_blend_from_meter: null handle");
    if (m->nch != a->nch || m->mode != a->mode || m->device != a->device)
        return fail(SDR_E_INVALID, "audio_blend_from_meter: the meter (nch %d, mode %d, device %d) is not the stage's (%d, %d, %d)",
                    m->nch, m->mode, m->device, a->nch, a->mode, a->device);
    return launch_on(a->device, k_audio_blend, groups256(a->nch), S(stream), m->rows, a->st, a->nch, (float)a->block_if,
                     (float)(a->block_if / 5), a->lo, a->hi - a->lo);
}

int sdr_audio_finish(sdr_audio* a, const int16_t* in, size_t in_stride, int16_t* out, size_t out_stride, void* stream) {
    if (!a || !in || !out) return fail(SDR_E_INVALID, "audio_finish: null argument");
    const size_t need = (size_t)a->width * a->n;
    if (in_stride < need || out_stride < need || (in_stride & 1) || (out_stride & 1))
        return fail(SDR_E_INVALID, "audio_finish: strides %zu, %zu must be even and >= width*n_audio = %zu", in_stride,
                    out_stride, need);
    if (((uintptr_t)in & 3) || ((uintptr_t)out & 3)) return fail(SDR_E_INVALID, "audio_finish: a base is not 4-byte aligned");
    HIP_TRY(hipSetDevice(a->device));
    AudioFinish q{};
    q.in = in;
    q.in_stride = in_stride;
    q.out = out;
    q.out_stride = out_stride;
    q.st = a->st;
    q.nch = a->nch;
    q.n = a->n;
    q.a = a->a;
    q.b = a->b;
    q.rn = 1.0f / (float)a->n;
    if (a->width == 2) launch_finish<2>(a->shape, a->nch, (hipStream_t)stream, q);
    else launch_finish<1>(a->shape, a->nch, (hipStream_t)stream, q);
    LAUNCH_CHECK();
    return SDR_OK;
}

int sdr_audio_read_state(sdr_audio* a, sdr_audio_state* host, void* stream) {
    if (!a || !host) return fail(SDR_E_INVALID, "audio_read_state: null argument");
    HIP_TRY(hipSetDevice(a->device));
    return copy_records(a->st, host, a->nch, S(stream));
}

}  // extern "C"
