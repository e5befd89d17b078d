// stage_device.h -- device code shared by the stage kernels (sdr_kernels.hip) and the context-free
// primitives (sdr_primitives.hip): the x86 float -> int16 conversion, the output stages' error words,
// the generic rational resampler and the clock-recovery argmax. Everything is in the unnamed
// namespace: a unit that includes it instantiates (with internal linkage) only the kernels it
// launches, so no kernel is compiled twice. Both units are built with -fno-slp-vectorize and
// `fp contract(off)`.
#pragma once

#include "sdr_internal.h"

namespace {

// static_cast<short>(float) as g++/x86-64 lowers it (mono.cpp:41, stereo.cpp:101-102):
// cvttss2si (INT_MIN when out of range or NaN), then the low 16 bits.
__device__ __forceinline__ int32_t cvt_i32_x86(float v) {
    return (v >= -2147483648.0f && v < 2147483648.0f) ? (int32_t)v : INT32_MIN;
}
__device__ __forceinline__ int16_t cvt_i16_x86(float v) {
    return (int16_t)(uint16_t)((uint32_t)cvt_i32_x86(v) & 0xFFFFu);
}

// The error words an output stage checks before it hands out a block (SDR_PCM_POISON audio, NaN
// rds_clean rows, nbits = SDR_NBITS_POISONED instead of outputs, include/sdr_amd.h):
//   pers  the persistent PLL launch that produced this block's phases (null for other blocks)
//   fail  the context's sticky release-timeout word: a producer overwrote a parity buffer whose
//         readers had not released it within the bounded wait (release_wait), so any reader that
//         runs after it may read the next block's data; set until sdr_ctx_reset.
struct Poison {
    const uint32_t* pers;
    const uint32_t* fail;
};
// read once per wave (scalar loads of kernel-argument addresses; the value is made wave-uniform)
__device__ __forceinline__ uint32_t poison_word(const Poison& p) {
    uint32_t v = 0;
    if (p.pers) v |= *p.pers;
    if (p.fail) v |= *p.fail;
    return __builtin_amdgcn_readfirstlane(v);
}
// The same words read again once the kernel's input loads have completed (issued after the staging
// barrier, consumed before the stores, so its latency hides behind the compute): a release wait that
// expires while a reader runs sets its word before the producer overwrites that reader's inputs, so
// a reader that loaded any overwritten sample sees the word here (agent-scope loads: from L2, the
// coherence point) and poisons instead of storing a mixed block.
__device__ __forceinline__ uint32_t poison_late(const Poison& p) {
    uint32_t v = 0;
    if (p.pers) v |= __hip_atomic_load(p.pers, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p.fail) v |= __hip_atomic_load(p.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return v;
}

// ------------------------------------------------------------------------------------------
// Rational resampler, filter.cpp:123-147. Output n: phase = nD mod U, q = (nD - phase)/U,
// y[n] = sum_j hp[phase][j] * x[q - j] (j ascending == k ascending), hp = polyphase taps,
// cnt[phase] = number of taps of that phase. The phase restarts every block (the reference
// recomputes it from n, :131). OUT: 0 -> f32 y, 1 -> int16(16384*y) (mono.cpp:40-42),
// 2 -> stereo L/R int16 from two inputs a (mono) and b (stereo) (stereo.cpp:100-107).
// ------------------------------------------------------------------------------------------
template <int OUT, int NTAP = 0>   // NTAP > 0: U == 1 with NTAP taps (uniform taps, unrolled sums)
__global__ __launch_bounds__(sdrk::BLK) void k_resample(const float* __restrict__ xa, const float* __restrict__ ha,
                                                        size_t xa_stride, size_t ha_stride,
                                                        const float* __restrict__ xb, const float* __restrict__ hb,
                                                        size_t xb_stride, size_t hb_stride,
                                                        const float* __restrict__ hp, const int* __restrict__ cnt,
                                                        int L, int U, int D, int ny, int tile, int hist_lo,
                                                        void* __restrict__ y, size_t y_stride) {
    constexpr int BLK = sdrk::BLK;
    extern __shared__ float4 smem4[];
    float* sa = reinterpret_cast<float*>(smem4);
    const int ch = blockIdx.y, tid = threadIdx.x;
    const int n0 = blockIdx.x * tile, n1 = min(n0 + tile, ny);
    const int qlo = (int)(((long long)n0 * D) / U) - L;   // smallest input index any output reads
    const int qhi = (int)(((long long)(n1 - 1) * D) / U);
    const int W = qhi - qlo + 1;
    const int Wp = (W + 3) & ~3;
    float* sb = sa + Wp;
    // staging: 4 loads per thread in flight per round
    auto stage = [&](float* dst, const float* xc, const float* hc) {
        for (int i0 = tid; i0 < W; i0 += 4 * BLK) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + u * BLK, m = qlo + i;
                v[u] = (i < W && m >= hist_lo) ? (m < 0 ? hc : xc)[m] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (i0 + u * BLK < W) dst[i0 + u * BLK] = v[u];
        }
    };
    stage(sa, xa + (size_t)ch * xa_stride, ha + (size_t)ch * ha_stride);
    if (OUT == 2) stage(sb, xb + (size_t)ch * xb_stride, hb + (size_t)ch * hb_stride);
    __syncthreads();
    for (int n = n0 + tid; n < n1; n += BLK) {
        const long long nd = (long long)n * D;
        const int ph = NTAP > 0 ? 0 : (int)(nd % U);
        const int q = NTAP > 0 ? (int)nd : (int)(nd / U);
        const float* hr = hp + (size_t)ph * L;
        const int base = q - qlo;
        float a = 0.0f, b = 0.0f;
        if (NTAP > 0) {                 // one polyphase row (U = 1): wave-uniform scalar taps
#pragma unroll 8
            for (int j = 0; j < NTAP; j++) {
                const float hj = hp[j];
                a = a + hj * sa[base - j];
                if (OUT == 2) b = b + hj * sb[base - j];
            }
        } else {
            const int c = cnt[ph];
            for (int j = 0; j < c; j++) {
                const float hj = hr[j];
                a = a + hj * sa[base - j];
                if (OUT == 2) b = b + hj * sb[base - j];
            }
        }
        if (OUT == 0) {
            static_cast<float*>(y)[(size_t)ch * y_stride + n] = a;
        } else if (OUT == 1) {
            static_cast<int16_t*>(y)[(size_t)ch * y_stride + n] = cvt_i16_x86(16384 * a);
        } else {
            int16_t* o = static_cast<int16_t*>(y) + (size_t)ch * y_stride + 2 * n;
            o[0] = cvt_i16_x86(16384 * (a + b));   // left  = 16384*(m + s)
            o[1] = cvt_i16_x86(16384 * (a - b));   // right = 16384*(m - s)
        }
    }
}

inline size_t resample_lds_bytes(int L, int U, int D, int tile, int ninputs) {
    const int W = (int)(((long long)tile * D) / U) + L + 2;
    return (size_t)ninputs * ((W + 3) & ~3) * sizeof(float) + 64;
}

// cdr(), rds_utilities.cpp:4-21: argmax over offsets i < sps of sum_k |(int)x[k*sps+i]|,
// first maximum wins, 0 when every sum is 0. One wave per channel, one lane per offset; the argmax
// is a wave reduction of (sum, -offset) over the sums > 0 (the reference's strict > from maxv = 0).
__device__ __forceinline__ int cdr_wave(const float* x, int n, int sps) {
    const int lane = threadIdx.x;
    const int nk = n / sps;
    unsigned long long key = 0;                     // (sum << 32) | ~offset of this lane's best offset
    for (int i = lane; i < sps; i += 64) {
        uint32_t s = 0;
        for (int k = 0; k < nk; k++) {
            const int32_t v = cvt_i32_x86(x[k * sps + i]);
            s += (uint32_t)(v < 0 ? -(uint32_t)v : (uint32_t)v);
        }
        const int32_t si = (int32_t)s;
        const unsigned long long ki = si > 0 ? ((unsigned long long)(uint32_t)si << 32) | (uint32_t)~(uint32_t)i : 0ull;
        if (ki > key) key = ki;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(key, m, 64);
        if (o > key) key = o;
    }
    return key ? (int)~(uint32_t)(key & 0xFFFFFFFFull) : 0;
}

}  // namespace
