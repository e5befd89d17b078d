// sdr_primitives.hip -- the context-free batched primitives of the C ABI (filter.cpp, demod.cpp,
// pll.cpp, rds_utilities.cpp over many channels) and the kernels that only they launch. Numerics
// as sdr_kernels.hip: f32 product then f32 add in tap order, no contraction.

#include "sdr_internal.h"

#include <algorithm>
#include <mutex>
#include <vector>

#include "pll_math.h"
#include "demod_phase.h"
#include "stage_device.h"

#pragma clang fp contract(off)

using namespace sdrk;

namespace {

// ------------------------------------------------------------------------------------------
// Decimating FIR, filter.cpp:106-121: y[n] = sum_{k<ntaps} h[k] * x[nD-k], ascending k, f32
// mul then add. x[m] for m < 0 comes from `hist` (hist[m], m >= -nhist). NT = 1 or 2 tap sets
// sharing one staged window. SQUARE: the input is x*x (rds.cpp:111-113 fused into :116).
// ------------------------------------------------------------------------------------------
template <int NT, bool SQUARE>
__global__ __launch_bounds__(BLK) void k_fir(const float* __restrict__ x, size_t x_stride,
                                             const float* __restrict__ hist, size_t hist_stride,
                                             const float* __restrict__ h0, const float* __restrict__ h1, int ntaps,
                                             int D, int ny, int tile, float* __restrict__ y0,
                                             float* __restrict__ y1, size_t y_stride,
                                             double* __restrict__ rx0, size_t rx_stride) {
    extern __shared__ float4 smem4[];
    float* sh = reinterpret_cast<float*>(smem4);
    const int ntaps_pad = (ntaps + 3) & ~3;
    const int ch = blockIdx.y, tid = threadIdx.x;
    const int n0 = blockIdx.x * tile, n1 = min(n0 + tile, ny);
    const int m0 = n0 * D - (ntaps - 1), m1 = (n1 - 1) * D;
    const int W = m1 - m0 + 1;
    float* sx = sh + NT * ntaps_pad;
    const float* xc = x + (size_t)ch * x_stride;
    const float* hc = hist + (size_t)ch * hist_stride;
    for (int i = tid; i < ntaps; i += BLK) {
        sh[i] = h0[i];
        if (NT == 2) sh[ntaps_pad + i] = h1[i];
    }
    for (int i = tid; i < W; i += BLK) {
        const int m = m0 + i;
        float v = (m < 0) ? hc[m] : xc[m];
        if (SQUARE) v = v * v;
        sx[i] = v;
    }
    __syncthreads();
    for (int n = n0 + tid; n < n1; n += BLK) {
        const int base = n * D - m0;
        float a0 = 0.0f, a1 = 0.0f;
        for (int k = 0; k < ntaps; k++) {
            const float v = sx[base - k];
            a0 = a0 + sh[k] * v;
            if (NT == 2) a1 = a1 + sh[ntaps_pad + k] * v;
        }
        y0[(size_t)ch * y_stride + n] = a0;
        if (NT == 2) y1[(size_t)ch * y_stride + n] = a1;
        if (rx0) rx0[(size_t)ch * rx_stride + n] = pllm::pll_rx(a0);   // y0 feeds a PLL: its reciprocal
    }
}

// state <- last nstate of x (filter.cpp:119 / :145) for the primitive entry points
__global__ void k_state_update(float* __restrict__ state, int nstate, const float* __restrict__ x,
                               size_t x_stride, int nx) {
    const int ch = blockIdx.x;
    float* s = state + (size_t)ch * nstate;
    const float* xc = x + (size_t)ch * x_stride;
    if (nx >= nstate) {
        for (int i = threadIdx.x; i < nstate; i += blockDim.x) s[i] = xc[nx - nstate + i];
    } else {
        // shift (single workgroup per channel: read all, barrier, write)
        for (int base = 0; base < nstate; base += blockDim.x) {
            const int i = base + threadIdx.x;
            float v = 0.0f;
            if (i < nstate) v = (i + nx < nstate) ? s[i + nx] : xc[i + nx - nstate];
            __syncthreads();
            if (i < nstate) s[i] = v;
            __syncthreads();
        }
    }
}

// fmDemodNoArctan over separate I/Q arrays (demod.cpp:3-24); prev updated by k_demod_prev.
// PH: the phase discriminator instead (sdr_fm_demod_phase, demod_phase.h).
template <bool PH>
__global__ __launch_bounds__(BLK) void k_demod(float* __restrict__ out, size_t out_stride,
                                               const float* __restrict__ I, const float* __restrict__ Q,
                                               size_t iq_stride, int n, const float2* __restrict__ prev) {
    const int ch = blockIdx.y;
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    const float* Ic = I + (size_t)ch * iq_stride;
    const float* Qc = Q + (size_t)ch * iq_stride;
    const float ci = Ic[i], cq = Qc[i];
    const float2 pv = (i == 0) ? prev[ch] : make_float2(Ic[i - 1], Qc[i - 1]);
    float r;
    if constexpr (PH) {
        float re, im;
        demod_products(f32x2{ci, cq}, f32x2{pv.x, pv.y}, re, im);
        r = demod_phase2(f32x2{re, re}, f32x2{im, im}).x;
    } else if ((ci == 0) & (cq == 0)) {
        r = 0.0f;
    } else {
        const float num = ci * (cq - pv.y) - cq * (ci - pv.x);
        const double den = (double)ci * (double)ci + (double)cq * (double)cq;
        r = (float)((double)num / den);
    }
    out[(size_t)ch * out_stride + i] = r;
}

__global__ void k_demod_prev(float2* __restrict__ prev, const float* __restrict__ I, const float* __restrict__ Q,
                             size_t iq_stride, int n, int nch) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch < nch) prev[ch] = make_float2(I[(size_t)ch * iq_stride + n - 1], Q[(size_t)ch * iq_stride + n - 1]);
}

// cdr(), rds_utilities.cpp:4-21 (stage_device.h cdr_wave): one wave per channel
__global__ __launch_bounds__(64) void k_cdr(int32_t* __restrict__ offset, const float* __restrict__ x,
                                            size_t x_stride, int n, int sps) {
    const int ch = blockIdx.x;
    const int off = cdr_wave(x + (size_t)ch * x_stride, n, sps);
    if (threadIdx.x == 0) offset[ch] = off;
}

// manchester_decode (rds_utilities.cpp:34-68), one lane per channel
__global__ void k_manchester(uint8_t* __restrict__ bits, size_t bits_stride, int32_t* __restrict__ nbits,
                             const uint8_t* __restrict__ symbols, size_t sym_stride,
                             const int32_t* __restrict__ nsym, int nch, int block_count,
                             int32_t* __restrict__ state) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= nch) return;
    const uint8_t* sy = symbols + (size_t)ch * sym_stride;
    uint8_t* bo = bits + (size_t)ch * bits_stride;
    const int m = nsym[ch];
    if (m <= 0) {            // an empty row consumes nothing: state and bits row stay (the reference
        nbits[ch] = 0;       // would read symbols[-1] when a half symbol is pending)
        return;
    }
    int half_symbol = state[2 * ch], start = state[2 * ch + 1];
    int nb = 0;
    if (start) bo[nb++] = (uint8_t)half_symbol;
    if (block_count == 0) {
        int score = 0;
        for (int i = 0; i < m - 1; i += 2) score += sy[i] ^ sy[i + 1];
        for (int j = 1; j < m - 1; j += 2) score -= sy[j] ^ sy[j + 1];
        start = score < 0;
    }
    for (int i = start; i < m - 1; i += 2) bo[nb++] = sy[i];
    if (((m - start) & 0x01) == 1) {
        half_symbol = sy[m - 1];
        start = 1;
    } else {
        start = 0;
    }
    state[2 * ch] = half_symbol;
    state[2 * ch + 1] = start;
    nbits[ch] = nb;
}

// differential_decode (rds_utilities.cpp:70-88), one lane per channel
__global__ void k_differential(uint8_t* __restrict__ out, size_t out_stride, const uint8_t* __restrict__ bits,
                               size_t bits_stride, const int32_t* __restrict__ nbits, int nch, int block_num,
                               int32_t* __restrict__ last_bit) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= nch) return;
    const int nb = nbits[ch];
    if (nb <= 0) return;
    const uint8_t* b = bits + (size_t)ch * bits_stride;
    uint8_t* o = out + (size_t)ch * out_stride;
    o[0] = (block_num == 0) ? b[0] : (uint8_t)(b[0] ^ (uint8_t)last_bit[ch]);
    for (int i = 1; i < nb; i++) o[i] = b[i] ^ b[i - 1];
    last_bit[ch] = b[nb - 1];
}

size_t fir_lds_bytes(int ntaps, int nt, int tile, int D) {
    const int ntaps_pad = (ntaps + 3) & ~3;
    const int W = (tile - 1) * D + ntaps;
    return (size_t)(nt * ntaps_pad + W + 4) * sizeof(float);
}

// polyphase tables of the taps the primitive resampler has been called with, keyed by (U, tap
// values): the reference's callers use a few fixed filters, so entries are kept (never freed
// under a kernel still in flight) and the set is only dropped, after a device sync, if it grows
struct PPEntry {
    int U = 0;
    std::vector<float> host;
    float* table = nullptr;
    int* cnt = nullptr;
    int L = 0;
};
struct PPCache {
    std::mutex m;
    std::vector<PPEntry> e;
};
PPCache g_pp;
constexpr size_t PP_CACHE_MAX = 16;

template <bool PH>
int fm_demod_launch(float* out, size_t out_stride, const float* I, const float* Q, size_t iq_stride, int nch, int n,
                    float* prev, void* stream) {
    if (!out || !I || !Q || !prev || nch <= 0 || n <= 0) return fail(SDR_E_INVALID, "fm_demod: bad arguments");
    hipLaunchKernelGGL(k_demod<PH>, dim3(cdiv(n, BLK), nch), dim3(BLK), 0, S(stream), out, out_stride, I, Q, iq_stride,
                       n, reinterpret_cast<const float2*>(prev));
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_demod_prev, dim3(cdiv(nch, 64)), dim3(64), 0, S(stream), reinterpret_cast<float2*>(prev), I,
                       Q, iq_stride, n, nch);
    LAUNCH_CHECK();
    return SDR_OK;
}

}  // namespace

extern "C" {

int sdr_convolve_fir(float* y, size_t y_stride, const float* x, size_t x_stride, int nch, int nx, const float* h,
                     int ntaps, float* state, int nstate, int D, void* stream) {
    if (!y || !x || !h || !state || nch <= 0 || nx <= 0 || ntaps <= 0 || D <= 0 || nstate < ntaps - 1)
        return fail(SDR_E_INVALID, "convolve_fir: bad arguments (nstate must be >= ntaps-1)");
    const int ny = nx / D;
    if (ny > 0) {
        const int tile = FIR_TILE;
        const size_t lds = fir_lds_bytes(ntaps, 1, tile, D);
        if (lds > 160 * 1024) return fail(SDR_E_INVALID, "convolve_fir: ntaps*D too large for one tile");
        hipLaunchKernelGGL((k_fir<1, false>), dim3(cdiv(ny, tile), nch), dim3(BLK), lds, S(stream), x, x_stride,
                           state + nstate, (size_t)nstate, h, nullptr, ntaps, D, ny, tile, y, nullptr, y_stride, nullptr, 0);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_state_update, dim3(nch), dim3(256), 0, S(stream), state, nstate, x, x_stride, nx);
    LAUNCH_CHECK();
    return SDR_OK;
}

int sdr_convolve_fir_resample(float* y, size_t y_stride, const float* x, size_t x_stride, int nch, int nx,
                              const float* h, int ntaps, float* state, int nstate, int U, int D, void* stream) {
    if (!y || !x || !h || !state || nch <= 0 || nx <= 0 || ntaps <= 0 || U <= 0 || D <= 0)
        return fail(SDR_E_INVALID, "convolve_fir_resample: bad arguments");
    const int ny = (int)(((long long)nx * U) / D);
    // polyphase table of the (device) taps; the taps are read on the caller's stream so that a
    // preceding asynchronous upload of them on that stream is complete
    std::vector<float> hh(ntaps);
    HIP_TRY(hipMemcpyAsync(hh.data(), h, ntaps * sizeof(float), hipMemcpyDeviceToHost, S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));
    std::lock_guard<std::mutex> lk(g_pp.m);
    const PPEntry* pe = nullptr;
    for (const PPEntry& e : g_pp.e)
        if (e.U == U && e.host == hh) { pe = &e; break; }
    if (!pe) {
        if (g_pp.e.size() >= PP_CACHE_MAX) {
            HIP_TRY(hipDeviceSynchronize());
            for (PPEntry& e : g_pp.e) { (void)hipFree(e.table); (void)hipFree(e.cnt); }
            g_pp.e.clear();
        }
        Polyphase pp = make_polyphase(hh, U);
        PPEntry ne;
        ne.U = U; ne.host = hh; ne.L = pp.L;
        HIP_TRY(hipMalloc(&ne.table, pp.table.size() * sizeof(float)));
        HIP_TRY(hipMalloc(&ne.cnt, pp.cnt.size() * sizeof(int)));
        HIP_TRY(hipMemcpy(ne.table, pp.table.data(), pp.table.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ne.cnt, pp.cnt.data(), pp.cnt.size() * sizeof(int), hipMemcpyHostToDevice));
        g_pp.e.push_back(std::move(ne));
        pe = &g_pp.e.back();
    }
    // the deepest look-back is output 0: x[-(ceil(ntaps/U)-1)] (100 in every mode)
    const int lookback = (ntaps + U - 1) / U - 1;
    if (nstate < lookback)
        return fail(SDR_E_INVALID, "convolve_fir_resample: nstate %d < look-back %d", nstate, lookback);
    if (ny > 0) {
        const int tile = 256;
        const size_t lds = resample_lds_bytes(pe->L, U, D, tile, 1);
        hipLaunchKernelGGL(k_resample<0>, dim3(cdiv(ny, tile), nch), dim3(BLK), lds, S(stream), x, state + nstate,
                           x_stride, (size_t)nstate, nullptr, nullptr, (size_t)0, (size_t)0, pe->table, pe->cnt,
                           pe->L, U, D, ny, tile, -nstate, (void*)y, y_stride);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_state_update, dim3(nch), dim3(256), 0, S(stream), state, nstate, x, x_stride, nx);
    LAUNCH_CHECK();
    return SDR_OK;
}

int sdr_fm_demod(float* out, size_t out_stride, const float* I, const float* Q, size_t iq_stride, int nch, int n,
                 float* prev, void* stream) {
    return fm_demod_launch<false>(out, out_stride, I, Q, iq_stride, nch, n, prev, stream);
}

int sdr_fm_demod_phase(float* out, size_t out_stride, const float* I, const float* Q, size_t iq_stride, int nch, int n,
                       float* prev, void* stream) {
    return fm_demod_launch<true>(out, out_stride, I, Q, iq_stride, nch, n, prev, stream);
}

int sdr_demod_coeffs(float* c, int max, int* n) {
    static const float k[SDR_DEMOD_K + 1] = {SDR_DEMOD_C0, SDR_DEMOD_C1, SDR_DEMOD_C2, SDR_DEMOD_C3,
                                             SDR_DEMOD_C4, SDR_DEMOD_C5, SDR_DEMOD_C6, SDR_DEMOD_C7};
    if (n) *n = SDR_DEMOD_K + 1;
    if (c && max >= SDR_DEMOD_K + 1)
        for (int i = 0; i <= SDR_DEMOD_K; i++) c[i] = k[i];
    return SDR_OK;
}

int sdr_fmpll(float* out, size_t out_stride, const float* in, size_t in_stride, int nch, int n, float freq, float Fs,
              sdr_pll_state* state, float ncoScale, float phaseAdjust, float normBandwidth, void* stream) {
    if (!out || !in || !state || nch <= 0 || n < 0) return fail(SDR_E_INVALID, "fmpll: bad arguments");
    const size_t ts = round_up((size_t)std::max(n, 1), 4);
    // scratch: input reciprocals (f64), phases and -in (f32), each [nch][ts]
    const size_t rx_bytes = ts * nch * sizeof(double), t_bytes = 2 * ts * nch * sizeof(float);
    hipStream_t s = S(stream);
    // one scratch buffer per stream, reused in that stream's order (buffers from the
    // stream-ordered pool, hipMallocAsync / hipFreeAsync per call, came back wrong)
    void* scratch = nullptr;
    std::unique_lock<std::mutex> lk(g_scratch_mu);   // held until the PLL kernels are enqueued
    {
        const int rc = stream_scratch(s, rx_bytes + t_bytes, &scratch);
        if (rc != SDR_OK) return rc;
    }
    double* rxbuf = static_cast<double*>(scratch);
    float* tbuf = reinterpret_cast<float*>(rxbuf + ts * nch);
    return launch_pll(false, in, in_stride, n, nch, freq, Fs, tbuf, ts, rxbuf, tbuf + ts * nch, out, out_stride,
                      state, ncoScale, phaseAdjust, normBandwidth, s);
}

int sdr_cdr(int32_t* offset, const float* x, size_t x_stride, int nch, int n, int sps, void* stream) {
    if (!offset || !x || nch <= 0 || n < 0 || sps <= 0 || sps > 64) return fail(SDR_E_INVALID, "cdr: bad arguments");
    hipLaunchKernelGGL(k_cdr, dim3(nch), dim3(64), 0, S(stream), offset, x, x_stride, n, sps);
    LAUNCH_CHECK();
    return SDR_OK;
}

int sdr_manchester_decode(uint8_t* bits, size_t bits_stride, int32_t* nbits, const uint8_t* symbols, size_t sym_stride,
                          const int32_t* nsym, int nch, int block_count, int32_t* state, void* stream) {
    if (!bits || !nbits || !symbols || !nsym || !state || nch <= 0) return fail(SDR_E_INVALID, "manchester: bad arguments");
    hipLaunchKernelGGL(k_manchester, dim3(cdiv(nch, 64)), dim3(64), 0, S(stream), bits, bits_stride, nbits, symbols,
                       sym_stride, nsym, nch, block_count, state);
    LAUNCH_CHECK();
    return SDR_OK;
}

int sdr_differential_decode(uint8_t* out, size_t out_stride, const uint8_t* bits, size_t bits_stride,
                            const int32_t* nbits, int nch, int block_num, int32_t* last_bit, void* stream) {
    if (!out || !bits || !nbits || !last_bit || nch <= 0) return fail(SDR_E_INVALID, "differential: bad arguments");
    hipLaunchKernelGGL(k_differential, dim3(cdiv(nch, 64)), dim3(64), 0, S(stream), out, out_stride, bits, bits_stride,
                       nbits, nch, block_num, last_bit);
    LAUNCH_CHECK();
    return SDR_OK;
}

}  // extern "C"
