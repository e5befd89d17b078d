// sdr_kernels.hip -- MI355X (gfx950) stage kernels of the FM/RDS DSP hot path and the stage calls of
// the C ABI that launch them (the context itself: sdr_ctx.hip; the persistent PLL launch's host
// side: sdr_plls.cpp; streams and test hooks: sdr_streams.hip; the context-free primitives:
// sdr_primitives.hip).
//
// Hot path of TheZxc07/real-time-SDR recast as batched kernels over many independent channels:
//   front end   u8 I/Q -> 101-tap FIR /10 on I and Q -> FM discriminator    rffrontend.cpp:58-71
//               (sdr_frontend.hip)
//   mono        101-tap resampler U/D -> int16                            mono.cpp:34-42
//   stereo      pilot BPF -> PLL(19k, x2) ; band BPF ; mixer ; delay ; 2 resamplers -> L/R
//                                                                          stereo.cpp:74-107
//   rds DSP     BPF -> square -> BPF -> PLL(114k, x0.5) ; delay ; mixer -> 247/640 resampler
//               -> RRC                                                     rds.cpp:105-133
//   rds bits    cdr -> slicer -> Manchester -> differential               rds.cpp:135-167
//   PLL / NCO   pll.cpp:4-61 (sdr_pll.hip)
//
// Numerics ("exact" mode, default): every kernel keeps the reference's rounding points --
// f32 product then f32 add in tap order (no contraction: `fp contract(off)` below), the
// discriminator's f64 denominator/division, the PLL's f64 atan2/sin/cos on f32 arguments.
// Layout: see sdr_internal.h.

#include "sdr_internal.h"

#include <algorithm>
#include <cstdint>
#include <vector>

#include "pll_math.h"
#include "nco.h"
#include "stage_device.h"

#pragma clang fp contract(off)

#ifndef SDR_FILL_FE_PARTS
#define SDR_FILL_FE_PARTS 0      // sdr_frontend_pre_parts: one front-end launch per part (A/B only)
#endif

using namespace sdrk;

namespace {

// ------------------------------------------------------------------------------------------
// The IF-rate 101-tap FIRs without decimation (filter.cpp:106-121 with D = 1: pilot/band BPFs
// stereo.cpp:74,80, RDS BPF rds.cpp:105, squared-RDS BPF :116, RRC :133), register-blocked:
// each thread computes FRB_R consecutive outputs from a window of FRB_R + 100 samples read once
// from LDS (16-byte reads), and every output still sums h[k] * x[n-k] in ascending k as an f32
// product then an f32 add (no contraction). NT tap sets (1..3) share one staged window: the stereo
// pilot and band filters and the RDS band filter all read fm_demod (stereo.cpp:74,80, rds.cpp:105).
// Taps are wave-uniform scalar operands, fetched FRB_TC at a time: scalar loads return out of
// order, so every wait for one is lgkmcnt(0); the next chunk is therefore requested only after the
// current chunk's first products have waited for it, and its latency hides behind the rest of the
// chunk (FRB_TC x R x NT multiply-adds) instead of stalling every tap.
// ------------------------------------------------------------------------------------------
constexpr int FRB_T = 101;                 // taps (rf_taps, project.cpp:61); FRB_R, FRB_TILE: sdr_internal.h
constexpr int FRB_W = FRB_TILE + FRB_T - 1 + 3;   // staged samples (+3: whole 16-byte reads)

// Up to three tap sets over one input window. Output t goes to y[t] (stride y_stride[t]); y[0] may
// also get its PLL reciprocals (rx0) and its negation (y0neg, same stride: the lane-pair PLL's
// second input, sdr_pll.hip pll_run_split), and y[2] the history of an extended stream (hist2_src:
// the other parity's row, copied in front by the first tile of each channel).
struct FirRb {
    const float* h[3];
    const float* h01;          // {h[0][k], h[1][k]} interleaved, padded to 104 pairs (k_fir_rb<3, *, true>)
    float* y[3];
    size_t y_stride[3];
    float* y0neg;
    double* rx0;
    size_t rx_stride;
    const float* hist2_src;
    Poison err;                // {null, null}, or the block's error words: NaN outputs when one is set
    float* ydup;              // non-null: y[0] stored here too (stride ydup_stride)
    size_t ydup_stride;
    int x0;                    // first tile (blockIdx.x + x0): a part of the block (sdr_frontend_pre_parts)
};

// PK (NT == 3): tap sets 0 and 1 (the stereo pilot and band BPFs) run as packed pairs -- one
// v_pk_mul_f32 + one v_pk_add_f32 per sample and output for both, the same two roundings each as
// filter.cpp:115 -- and set 2 (the RDS BPF) scalar: 4 VALU per sample and output instead of 6.
template <int NT, bool SQUARE, bool PK = false>
__global__ __launch_bounds__(BLK) void k_fir_rb(const float* __restrict__ x, size_t x_stride,
                                                const float* __restrict__ hist, size_t hist_stride, int ny,
                                                const FirRb f) {
    static_assert(!PK || NT >= 2, "packed pairs: sets 0 and 1 of a 2- or 3-set pass");
    constexpr int T = FRB_T, R = FRB_R;
    __shared__ __attribute__((aligned(16))) float sx[(FRB_W + 3) & ~3];
    __shared__ uint32_t s_poison;                                 // one decision per workgroup
    const int ch = blockIdx.y, tid = threadIdx.x;
    const bool checks = f.err.pers || f.err.fail;
    if (checks && tid == 0) s_poison = poison_word(f.err);        // (its latency hides behind the staging)
    const int xt = (int)blockIdx.x + f.x0;                        // tile of the block
    const int n0 = xt * FRB_TILE;
    const int m0 = n0 - (T - 1);
    const int W = min(FRB_TILE, ny - n0) + T - 1;
    {
        // all loads of the tile in flight at once, then the LDS writes
        const float* xc = x + (size_t)ch * x_stride;
        const float* hc = hist + (size_t)ch * hist_stride;
        constexpr int NL = (FRB_TILE + FRB_T - 1 + BLK - 1) / BLK;
        float v[NL];
#pragma unroll
        for (int u = 0; u < NL; u++) {
            const int i = tid + u * BLK, m = m0 + i;
            v[u] = (i < W) ? (m < 0 ? hc : xc)[m] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < NL; u++) {
            const int i = tid + u * BLK;
            if (i < W) sx[i] = SQUARE ? v[u] * v[u] : v[u];       // rds.cpp:111-113
        }
    }
    if (NT == 3 && f.hist2_src && xt == 0 && tid < HIST)          // y[2]'s history (extended stream)
        f.y[2][(size_t)ch * f.y_stride[2] + tid - HIST] = f.hist2_src[(size_t)ch * f.y_stride[2] + ny - HIST + tid];
    __syncthreads();
    const int nb = n0 + tid * R;
    if (nb >= ny) return;
    const uint32_t late = checks ? poison_late(f.err) : 0u;     // after every input load of the tile
    // w[i] = x[nb - (T-1) + i]; output nb + j at tap k reads w[j + T-1 - k] (samples past the
    // staged window only feed outputs >= ny, which are not stored)
    float w[R + T - 1 + 3];
#pragma unroll
    for (int i = 0; i < (R + T - 1 + 3) / 4; i++) {
        const float4 v = reinterpret_cast<const float4*>(sx + tid * R)[i];
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    float a[NT][R];
    constexpr int FRB_TC = 4;
    constexpr int FRB_NC = (FRB_T + FRB_TC - 1) / FRB_TC;   // chunks (tap buffers are padded past 101)
    typedef float f4v __attribute__((ext_vector_type(FRB_TC)));
    if constexpr (PK) {
        typedef float f8v __attribute__((ext_vector_type(2 * FRB_TC)));
        constexpr bool S2 = NT == 3;                     // a third, scalar set beside the pair
        f32x2 a01[R];
        float a2[R];
#pragma unroll
        for (int j = 0; j < R; j++) { a01[j] = f32x2{0.0f, 0.0f}; a2[j] = 0.0f; }
        f8v pb[2];                                       // {h0, h1} pairs of chunk c in pb[c & 1]
        f4v sb[2] = {};                                  // set 2's taps of chunk c
        auto load8 = [&](f8v& d, int c) {
            asm volatile("s_load_dwordx8 %0, %1, %2" : "=s"(d) : "s"(f.h01), "s"(c * FRB_TC * 8) : "memory");
        };
        auto load4 = [&](f4v& d, int c) {
            if constexpr (S2)
                asm volatile("s_load_dwordx4 %0, %1, %2" : "=s"(d) : "s"(f.h[NT - 1]), "s"(c * FRB_TC * 4) : "memory");
        };
        load8(pb[0], 0);
        load4(sb[0], 0);
        // the wait redefines the loaded registers, so no use of them is scheduled above it (a
        // product hoisted above a plain waitcnt read the taps before they landed)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(pb[0]), "+s"(sb[0]) :: "memory");
#pragma unroll
        for (int c = 0; c < FRB_NC; c++) {
#pragma unroll
            for (int kk = 0; kk < FRB_TC; kk++) {
                const int k = c * FRB_TC + kk;
                if (k < T) {
                    const double hp = __builtin_bit_cast(double, f32x2{pb[c & 1][2 * kk], pb[c & 1][2 * kk + 1]});
#pragma unroll
                    for (int j = 0; j < R; j++) {
                        const int i = j + T - 1 - k;
                        // plain vector code: the compiler broadcasts the sample by op_sel (no copy)
                        // and knows the packed result's latency (no inline-asm wait state, unlike an
                        // inline-asm v_pk_mul_f32)
                        const f32x2 pr = __builtin_bit_cast(f32x2, hp) * f32x2{w[i], w[i]};
                        a01[j] = a01[j] + pr;                                  // filter.cpp:115
                        if constexpr (S2) a2[j] = a2[j] + sb[c & 1][kk] * w[i];
                    }
                }
                if (kk == 0 && c + 1 < FRB_NC) {
                    __builtin_amdgcn_sched_barrier(0);
                    load8(pb[(c + 1) & 1], c + 1);
                    load4(sb[(c + 1) & 1], c + 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (c + 1 < FRB_NC) {
                __builtin_amdgcn_sched_barrier(0);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(pb[(c + 1) & 1]), "+s"(sb[(c + 1) & 1]) :: "memory");
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int j = 0; j < R; j++) {
            a[0][j] = a01[j].x;
            a[1][j] = a01[j].y;
            if constexpr (S2) a[NT - 1][j] = a2[j];
        }
    } else {
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int j = 0; j < R; j++) a[t][j] = 0.0f;
    // taps: scalar loads issued by hand (the compiler would wait for every outstanding scalar load
    // at each tap's first use), one chunk of FRB_TC taps per tap set ahead
    f4v buf[2][NT];                                     // chunk c in buf[c & 1]
    // base address in an SGPR pair, byte offset in an SGPR (not one address pair per chunk)
    auto load = [&](f4v& d, const float* hp, int c) {
        asm volatile("s_load_dwordx4 %0, %1, %2" : "=s"(d) : "s"(hp), "s"(c * FRB_TC * 4) : "memory");
    };
#pragma unroll
    for (int t = 0; t < NT; t++) load(buf[0][t], f.h[t], 0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int t = 0; t < NT; t++) asm volatile("" : "+s"(buf[0][t]));   // no tap use above the wait
#pragma unroll
    for (int c = 0; c < FRB_NC; c++) {
#pragma unroll
        for (int kk = 0; kk < FRB_TC; kk++) {
            const int k = c * FRB_TC + kk;
            if (k < T) {
#pragma unroll
                for (int j = 0; j < R; j++) {
                    const float v = w[j + T - 1 - k];
#pragma unroll
                    for (int t = 0; t < NT; t++) a[t][j] = a[t][j] + buf[c & 1][t][kk] * v;   // filter.cpp:115
                    // the MACs stay scalar (this unit is built with -fno-slp-vectorize): packed f32 ops
                    // run at half rate (tools/microbench/valu_rate.hip), and pairing neighbouring
                    // outputs costs register realignment and occupancy
                }
            }
            if (kk == 0 && c + 1 < FRB_NC) {
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < NT; t++) load(buf[(c + 1) & 1][t], f.h[t], c + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (c + 1 < FRB_NC) {
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // chunk c + 1 landed
#pragma unroll
            for (int t = 0; t < NT; t++) asm volatile("" : "+s"(buf[(c + 1) & 1][t]));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    }
    // every sum is complete here: otherwise the compiler sinks the second and third tap sets' products
    // past the first set's (divergent) stores and spills their taps from SGPRs
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int j = 0; j < R; j++) asm volatile("" : "+v"(a[t][j]));
    if (checks && (s_poison | __builtin_amdgcn_readfirstlane(late)) != 0u) {   // no valid input behind this block
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int j = 0; j < R; j++) a[t][j] = __builtin_nanf("");
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
        float* o = f.y[t] + (size_t)ch * f.y_stride[t] + nb;
        if (nb + R <= ny) {
#pragma unroll
            for (int j = 0; j < R; j += 4)
                reinterpret_cast<float4*>(o + j)[0] = make_float4(a[t][j], a[t][j + 1], a[t][j + 2], a[t][j + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < R; j++)
                if (nb + j < ny) o[j] = a[t][j];
        }
    }
    if (f.ydup) {                                                 // a second copy of y[0]
        float* o = f.ydup + (size_t)ch * f.ydup_stride + nb;
        if (nb + R <= ny) {
#pragma unroll
            for (int j = 0; j < R; j += 4)
                reinterpret_cast<float4*>(o + j)[0] = make_float4(a[0][j], a[0][j + 1], a[0][j + 2], a[0][j + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < R; j++)
                if (nb + j < ny) o[j] = a[0][j];
        }
    }
    if (f.y0neg) {                                                // y[0] feeds a PLL: -y[0]
        float* o = f.y0neg + (size_t)ch * f.y_stride[0] + nb;
        if (nb + R <= ny) {
#pragma unroll
            for (int j = 0; j < R; j += 4)
                reinterpret_cast<float4*>(o + j)[0] = make_float4(-a[0][j], -a[0][j + 1], -a[0][j + 2], -a[0][j + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < R; j++)
                if (nb + j < ny) o[j] = -a[0][j];
        }
    }
    if (f.rx0) {                                                  // y[0] feeds a PLL: its reciprocal
        double* r = f.rx0 + (size_t)ch * f.rx_stride + nb;
        if (nb + R <= ny) {
#pragma unroll
            for (int j = 0; j < R; j += 2)
                reinterpret_cast<double2*>(r + j)[0] = make_double2(pllm::pll_rx(a[0][j]), pllm::pll_rx(a[0][j + 1]));
        } else {
#pragma unroll
            for (int j = 0; j < R; j++)
                if (nb + j < ny) r[j] = pllm::pll_rx(a[0][j]);
        }
    }
}

// ------------------------------------------------------------------------------------------
// The RDS 247/640 resampler (rds.cpp:130 -> filter.cpp:123-147) with lanes = channels: a
// workgroup takes 64 channels x RLC_TN outputs. Every output has its own polyphase row, shared by
// all 64 channels, so the rows of the tile are staged once in LDS and read as broadcasts, while
// each lane reads its own channel's samples from an odd-strided LDS tile (no bank conflicts).
// ptq[n] = (q << 8) | phase with phase = nD mod U, q = nD / U (host table; U < 256). Sums stay
// in ascending j (= ascending k of the reference) as f32 product then f32 add.
// ------------------------------------------------------------------------------------------
// outputs per workgroup, over 8 waves of 4 outputs: the x tile (64 channels x the tile's q span,
// 46 KB of LDS) bounds a CU to 2-3 workgroups, so 8 waves per workgroup instead of 4 give 16 waves per
// CU instead of 12 to hide the tap rows' scalar-load latency: 44.5 -> 37.7 us isolated. 16 outputs
// per workgroup (4 waves) or the tap rows by vector loads (lc_group_v, in order, 2 chunks ahead)
// were slower: 45.2, 59.5 us (profiles/r05/resample_lc_ab.txt).
constexpr int RLC_TN = 32;
constexpr int RLC_BLK = 64 * 8;   // threads per workgroup
constexpr int RLC_XL = 3;      // staged samples per lane and row: 64 * 3 >= the q span + look-back
constexpr int RLC_HL = 2;      // staged taps per lane and polyphase row: 64 * 2 >= L4

// four outputs of the 247/640 resampler whose q offsets from the first are (0, D1, D2, D3):
// acc[k] = sum_{j<101} hr[k*L4 + j] * x[q_k - j] in ascending j, x[q_0 - 100 + i] = xr[i]
template <int D1, int D2, int D3>
__device__ __forceinline__ void lc_group(const float* __restrict__ xr, const float* __restrict__ hr, int L4,
                                         float (&acc)[4]) {
    constexpr int NW = D3 + 101;
    constexpr int DK[4] = {0, D1, D2, D3};
    float w[NW];
#pragma unroll
    for (int i = 0; i < NW; i++) w[i] = xr[i];
#pragma unroll
    for (int k = 0; k < 4; k++) acc[k] = 0.0f;
    // taps of the 4 rows, 4 at a time (16-byte broadcasts), one chunk ahead; the barriers keep the
    // scheduler from hoisting every chunk's reads (4 x 104 registers) to the top
    float4 cur[4], nxt[4];
#pragma unroll
    for (int k = 0; k < 4; k++) cur[k] = *reinterpret_cast<const float4*>(hr + k * L4);
#pragma unroll
    for (int j0 = 0; j0 < 104; j0 += 4) {
        if (j0 + 4 < 104) {
#pragma unroll
            for (int k = 0; k < 4; k++) nxt[k] = *reinterpret_cast<const float4*>(hr + k * L4 + j0 + 4);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float hv[4] = {cur[k].x, cur[k].y, cur[k].z, cur[k].w};
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                const int j = j0 + jj;
                if (j < 101) acc[k] = acc[k] + hv[jj] * w[DK[k] + 100 - j];     // filter.cpp:139-141
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 4; k++) cur[k] = nxt[k];
    }
}

// The same four outputs with the tap rows read by hand-issued scalar loads from the polyphase table
// (hr[k]: row of output k, wave-uniform) instead of LDS broadcasts: the rows are wave-uniform
// operands, so they need no LDS (the tile's x window alone fits three workgroups per CU instead of
// two) and no LDS bandwidth (the 16-byte broadcasts were most of the kernel's LDS traffic). Chunks
// of 4 taps of the 4 rows, one chunk ahead (scalar loads return out of order: every wait is
// lgkmcnt(0), as in k_fir_rb).
template <int D1, int D2, int D3>
__device__ __forceinline__ void lc_group_s(const float* __restrict__ xr, const float* h0, const float* h1,
                                           const float* h2, const float* h3, float (&acc)[4]) {
    constexpr int NW = D3 + 101;
    constexpr int DK[4] = {0, D1, D2, D3};
    constexpr int TC = 4, NC = 104 / TC;                   // rows padded past 101 (the table has slack)
    typedef float f4v __attribute__((ext_vector_type(TC)));
    float w[NW];
#pragma unroll
    for (int i = 0; i < NW; i++) w[i] = xr[i];
#pragma unroll
    for (int k = 0; k < 4; k++) acc[k] = 0.0f;
    const float* hr[4] = {h0, h1, h2, h3};
    f4v buf[2][4];
    auto load = [&](f4v& d, const float* hp, int c) {
        asm volatile("s_load_dwordx4 %0, %1, %2" : "=s"(d) : "s"(hp), "s"(c * TC * 4) : "memory");
    };
#pragma unroll
    for (int k = 0; k < 4; k++) load(buf[0][k], hr[k], 0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int k = 0; k < 4; k++) asm volatile("" : "+s"(buf[0][k]));   // no tap use above the wait
#pragma unroll
    for (int c = 0; c < NC; c++) {
#pragma unroll
        for (int kk = 0; kk < TC; kk++) {
            const int j = c * TC + kk;
            if (j < 101) {
#pragma unroll
                for (int k = 0; k < 4; k++) acc[k] = acc[k] + buf[c & 1][k][kk] * w[DK[k] + 100 - j];   // filter.cpp:139-141
            }
            if (kk == 0 && c + 1 < NC) {
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < 4; k++) load(buf[(c + 1) & 1][k], hr[k], c + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (c + 1 < NC) {
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // chunk c + 1 landed
#pragma unroll
            for (int k = 0; k < 4; k++) asm volatile("" : "+s"(buf[(c + 1) & 1][k]));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) asm volatile("" : "+v"(acc[k]));
}

template <int NTAP>   // > 0: every polyphase row has exactly NTAP taps (fully unrolled sums)
__global__ __launch_bounds__(RLC_BLK) void k_resample_lc(const float* __restrict__ x, size_t x_stride, int hist_lo,
                                                     const float* __restrict__ hp, const int* __restrict__ cnt,
                                                     int L, const int* __restrict__ ptq, int ny, int nch,
                                                     float* __restrict__ y, size_t y_stride) {
    extern __shared__ float4 smem4[];
    float* smem = reinterpret_cast<float*>(smem4);
    constexpr int PW = RLC_TN / (RLC_BLK / 64);              // outputs per wave
    const int c0 = blockIdx.y * 64, n0 = blockIdx.x * RLC_TN;
    const int nn = min(RLC_TN, ny - n0);
    // wave index as a scalar: the per-output table reads (ptq, cnt) are then scalar loads issued
    // together, not vector loads each waiting for every load before it
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int qlo = (ptq[n0] >> 8) - (L - 1);
    const int W = (ptq[n0 + nn - 1] >> 8) - qlo + 1;
    const int SW = W | 1;
    const int L4 = (L + 3) & ~3;
    // NTAP == 101: the tap rows come from the table by scalar loads (lc_group_s), not from LDS
    constexpr bool STAGE_TAPS = NTAP != 101;
    float* sx = smem;                                        // [64][SW]
    float* sh = smem + ((64 * SW + 3) & ~3);                 // [RLC_TN][L4] (STAGE_TAPS)
    // staging with every load of a wave in flight before its LDS writes: rows c = wave + 4u of the
    // x tile (lanes along the row, RLC_XL loads per row), then the polyphase rows of the outputs
    {
        constexpr int NR = 64 / (RLC_BLK / 64);
        float v[NR][RLC_XL];
#pragma unroll
        for (int u = 0; u < NR; u++) {
            const int ch = min(c0 + wave + u * (RLC_BLK / 64), nch - 1);
            const float* xc = x + (size_t)ch * x_stride;
#pragma unroll
            for (int k = 0; k < RLC_XL; k++) {
                const int i = lane + 64 * k, m = qlo + i;
                v[u][k] = (i < W && m >= hist_lo) ? xc[m] : 0.0f;
            }
        }
        // the polyphase rows' loads go out with the x tile's, before any LDS write waits for them
        // (one round of global-memory latency per workgroup instead of two)
        float hv[PW][RLC_HL];
        if (STAGE_TAPS) {
#pragma unroll
            for (int o8 = 0; o8 < PW; o8++) {
                const int o = min(wave * PW + o8, nn - 1);
                const int ph = ptq[n0 + o] & 255;
                const int cn = cnt[ph];
#pragma unroll
                for (int k = 0; k < RLC_HL; k++) {
                    const int j = lane + 64 * k;
                    hv[o8][k] = (j < cn) ? hp[(size_t)ph * L + j] : 0.0f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < NR; u++) {
            const int c = wave + u * (RLC_BLK / 64);
#pragma unroll
            for (int k = 0; k < RLC_XL; k++) {
                const int i = lane + 64 * k;
                if (i < W) sx[c * SW + i] = v[u][k];
            }
        }
        if (STAGE_TAPS) {
#pragma unroll
            for (int o8 = 0; o8 < PW; o8++) {
                const int o = wave * PW + o8;
#pragma unroll
                for (int k = 0; k < RLC_HL; k++) {
                    const int j = lane + 64 * k;
                    if (o < nn && j < L4) sh[o * L4 + j] = hv[o8][k];
                }
            }
        }
    }
    __syncthreads();
    const int ch = c0 + lane;
    float out[PW];
    if (NTAP == 101) {
        // groups of 4 consecutive outputs from one register window: their q offsets (q_k - q_0) follow
        // one of four patterns for the 247/640 ratio (the fraction of 640 n / 247 picks it), a
        // wave-uniform branch into statically indexed code; the window is read from LDS once per
        // group (109 samples for 4 outputs instead of 4 x 101) and each tap row as 16-byte broadcasts
        static_assert(PW % 4 == 0, "whole groups");
#pragma unroll
        for (int g = 0; g < PW / 4; g++) {
            const int o = wave * PW + 4 * g;
            bool done = false;
            if (o + 3 < nn) {
                const int q0 = ptq[n0 + o] >> 8;
                const int d1 = (ptq[n0 + o + 1] >> 8) - q0, d2 = (ptq[n0 + o + 2] >> 8) - q0,
                          d3 = (ptq[n0 + o + 3] >> 8) - q0;
                const float* xr = sx + lane * SW + (q0 - qlo) - 100;   // xr[i] = x[q0 - 100 + i]
                // the 4 outputs' polyphase rows in the table (wave-uniform addresses)
                const float* h0 = hp + (size_t)__builtin_amdgcn_readfirstlane((ptq[n0 + o] & 255) * L);
                const float* h1 = hp + (size_t)__builtin_amdgcn_readfirstlane((ptq[n0 + o + 1] & 255) * L);
                const float* h2 = hp + (size_t)__builtin_amdgcn_readfirstlane((ptq[n0 + o + 2] & 255) * L);
                const float* h3 = hp + (size_t)__builtin_amdgcn_readfirstlane((ptq[n0 + o + 3] & 255) * L);
                float acc4[4];
                done = true;
                if (d1 == 3 && d2 == 5 && d3 == 8) lc_group_s<3, 5, 8>(xr, h0, h1, h2, h3, acc4);
                else if (d1 == 2 && d2 == 5 && d3 == 7) lc_group_s<2, 5, 7>(xr, h0, h1, h2, h3, acc4);
                else if (d1 == 2 && d2 == 5 && d3 == 8) lc_group_s<2, 5, 8>(xr, h0, h1, h2, h3, acc4);
                else if (d1 == 3 && d2 == 6 && d3 == 8) lc_group_s<3, 6, 8>(xr, h0, h1, h2, h3, acc4);
                else done = false;
                if (done) {
#pragma unroll
                    for (int k = 0; k < 4; k++) out[4 * g + k] = acc4[k];
                }
            }
            if (!done) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float acc = 0.0f;
                    if (o + k < nn) {
                        const int e = ptq[n0 + o + k];
                        const float* xr = sx + lane * SW + ((e >> 8) - qlo);
                        const float* hr = hp + (size_t)(e & 255) * L;   // (the table: taps are not staged)
                        for (int j = 0; j < 101; j++) acc = acc + hr[j] * xr[-j];
                    }
                    out[4 * g + k] = acc;
                }
            }
        }
    } else
#pragma unroll
    for (int o8 = 0; o8 < PW; o8++) {
        const int o = wave * PW + o8;
        float acc = 0.0f;
        if (o < nn) {
            const int e = ptq[n0 + o];
            const int cn = cnt[e & 255];
            const float* xr = sx + lane * SW + ((e >> 8) - qlo);  // x[q - j] = xr[-j]
            const float* hr = sh + o * L4;
            if (NTAP > 0) {
#pragma unroll
                for (int j = 0; j < NTAP; j++) acc = acc + hr[j] * xr[-j];
            } else {
            int j = 0;
            for (; j + 4 <= cn; j += 4) {
                const float4 h4 = *reinterpret_cast<const float4*>(hr + j);
                acc = acc + h4.x * xr[-j];
                acc = acc + h4.y * xr[-j - 1];
                acc = acc + h4.z * xr[-j - 2];
                acc = acc + h4.w * xr[-j - 3];
            }
            for (; j < cn; j++) acc = acc + hr[j] * xr[-j];
            }
        }
        out[o8] = acc;
    }
    if (ch < nch) {
        float* yo = y + (size_t)ch * y_stride + n0 + wave * PW;
        const int m = min(PW, nn - wave * PW);
#pragma unroll
        for (int o8 = 0; o8 < PW; o8++)
            if (o8 < m) yo[o8] = out[o8];
    }
}

int resample_lc_span(int L, int U, int D) {   // samples a tile reads: q span + look-back
    return (int)(((long long)(RLC_TN - 1) * D + U - 1) / U) + 1 + L;
}

size_t resample_lc_lds_bytes(int L, int U, int D, bool stage_taps) {
    const int W = resample_lc_span(L, U, D);
    return (size_t)((((64 * (W | 1)) + 3) & ~3) + (stage_taps ? RLC_TN * ((L + 3) & ~3) : 0)) * sizeof(float);
}

// ------------------------------------------------------------------------------------------
// Audio resamplers with U == 1 (mode 0: D = 5, mode 1: D = 9; filter.cpp:123-147 with one
// polyphase row of 101 taps), register-blocked: a thread computes AR consecutive outputs from a
// window of D*(AR-1) + 101 samples read once from LDS, the taps are scalar operands fetched in
// chunks of 4 by hand-issued scalar loads (as k_fir_rb), and every output sums h[j] * x[nD - j] in
// ascending j as an f32 product then an f32 add.
// ------------------------------------------------------------------------------------------
constexpr int AR = 4;                       // audio outputs per thread
constexpr int AT = 128;                     // threads per workgroup
constexpr int ATILE = AR * AT;              // audio outputs per workgroup

// acc[r] = sum_{j<101} h[j] * w[D*r + 100 - j] (ascending j), h wave-uniform
template <int D, int NW>
__device__ __forceinline__ void audio_mac(const float* __restrict__ h, const float (&w)[NW], float (&acc)[AR]) {
    constexpr int T = 101, TC = 4, NC = (T + TC - 1) / TC;   // tap buffers are padded past 101
    typedef float f4v __attribute__((ext_vector_type(TC)));
    f4v buf[2];
    auto load = [&](f4v& d, int c) {
        asm volatile("s_load_dwordx4 %0, %1, %2" : "=s"(d) : "s"(h), "s"(c * TC * 4) : "memory");
    };
#pragma unroll
    for (int r = 0; r < AR; r++) acc[r] = 0.0f;
    load(buf[0], 0);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(buf[0]) :: "memory");   // no tap use above the wait
#pragma unroll
    for (int c = 0; c < NC; c++) {
#pragma unroll
        for (int kk = 0; kk < TC; kk++) {
            const int j = c * TC + kk;
            if (j < T) {
#pragma unroll
                for (int r = 0; r < AR; r++) acc[r] = acc[r] + buf[c & 1][kk] * w[D * r + T - 1 - j];
            }
            if (kk == 0 && c + 1 < NC) {
                __builtin_amdgcn_sched_barrier(0);
                load(buf[(c + 1) & 1], c + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (c + 1 < NC) {
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(buf[(c + 1) & 1]) :: "memory");
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int r = 0; r < AR; r++) asm volatile("" : "+v"(acc[r]));
}

// thread tid's window of a tile staged at s (16-byte aligned: D*AR*tid floats in)
template <int D, int NW>
__device__ __forceinline__ void audio_window(const float* __restrict__ s, int tid, float (&w)[NW]) {
    static_assert((D * AR) % 4 == 0 && NW % 4 == 0, "16-byte LDS reads");
    const float4* p = reinterpret_cast<const float4*>(s + D * AR * tid);
#pragma unroll
    for (int i = 0; i < NW / 4; i++) {
        const float4 v = p[i];
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
}

template <int D>
constexpr int audio_win() { return D * (ATILE - 1) + 101; }         // staged samples per tile
template <int D>
constexpr int audio_tw() { return (D * (AR - 1) + 101 + 3) / 4 * 4; }   // window of one thread

// mono (mono.cpp:34-42): audio = short(16384 * resample(fm_demod))
template <int D>
__global__ __launch_bounds__(AT) void k_mono_out(const float* __restrict__ fm, size_t fm_stride,
                                                 const float* __restrict__ h, int n, int ny,
                                                 int16_t* __restrict__ audio, size_t audio_stride,
                                                 const Poison err) {
    constexpr int WIN = audio_win<D>(), TW = audio_tw<D>();
    __shared__ __attribute__((aligned(16))) float sa[(WIN + 3) / 4 * 4 + 4];
    __shared__ uint32_t s_poison;                            // one decision per workgroup
    const int ch = blockIdx.y, tid = threadIdx.x;
    if (tid == 0) s_poison = poison_word(err);
    const int o0 = blockIdx.x * ATILE;
    const int m0 = D * o0 - 100;
    const float* x = fm + (size_t)ch * fm_stride;
    const int kend = min(WIN, n - m0);                       // staged slots past the block feed only outputs >= ny
    {
        constexpr int NL = (WIN + AT - 1) / AT;              // every load of the tile in flight at once
        float v[NL];
#pragma unroll
        for (int u = 0; u < NL; u++) {
            const int k = tid + u * AT;
            v[u] = k < kend ? x[m0 + k] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < NL; u++)
            if (tid + u * AT < WIN) sa[tid + u * AT] = v[u];
    }
    __syncthreads();
    const int ob = o0 + tid * AR;
    if (ob >= ny) return;
    int16_t* o = audio + (size_t)ch * audio_stride + ob;
    if (s_poison != 0u) {        // fm_demod may hold another block's samples (a release wait timed out)
#pragma unroll
        for (int r = 0; r < AR; r++)
            if (ob + r < ny) o[r] = SDR_PCM_POISON;
        return;
    }
    const uint32_t late = poison_late(err);                  // after every input load of the tile
    float w[TW], acc[AR];
    audio_window<D>(sa, tid, w);
    audio_mac<D>(h, w, acc);
    const bool bad = __builtin_amdgcn_readfirstlane(late) != 0u;
#pragma unroll
    for (int r = 0; r < AR; r++)
        if (ob + r < ny) o[r] = bad ? (int16_t)SDR_PCM_POISON : cvt_i16_x86(16384 * acc[r]);   // mono.cpp:41
}

// ------------------------------------------------------------------------------------------
// Stereo post stage in one pass (stereo.cpp:83-107, U == 1). The staging of an audio tile
// computes, for every IF sample of its window, the 38 kHz carrier from the PLL phase (pll.cpp:52;
// carrier[0] is the previous block's last), the mixer product stereo_dc = RN32(2.0 * band *
// carrier) in f64 (stereo.cpp:83-85), and the mono delay fm[i - 50] (the 101-tap APF of :88 is
// an exact 50-sample shift); each thread then runs both resamplers over its register windows and
// writes L = short(16384 (m + s)), R = short(16384 (m - s)) (:100-107). The carrier and stereo_dc
// rows never reach HBM: only stereo_dc's last HIST samples (the next block's resampler history)
// and carrier[n] (the next block's carrier[0], and pllblock_args.lastCarrier) are stored.
// ------------------------------------------------------------------------------------------
struct StereoOut {
    const float* fm;            // this parity's fm_demod, extended (fm[-HIST..n))
    const float* band;          // band BPF output of this parity
    const float* t;             // PLL phases of this parity
    size_t fm_stride, plain_stride;
    float* car;                 // carrier rows of this parity: [ch][n] written
    const float* car_prev;      // the previous parity's: [ch][n] read
    size_t car_stride;
    sdr_pll_state* st;
    float ncoScale, phaseAdjust;
    float* sdc;                 // stereo_dc rows of this parity: the tail [n - HIST, n) written
    const float* sdc_prev;      // the previous parity's tail: this block's history
    size_t sdc_stride;
    const float* h;             // the 101 audio taps
    int n, ny;
    int16_t* lr;
    size_t lr_stride;
    Poison err;                 // the block's error words (persistent PLL launch, release timeout)
};

template <int D>
__global__ __launch_bounds__(AT) void k_stereo_out(const StereoOut a) {
    constexpr int WIN = audio_win<D>(), TW = audio_tw<D>();
    __shared__ __attribute__((aligned(16))) float sa[(WIN + 3) / 4 * 4 + 4];
    __shared__ __attribute__((aligned(16))) float sb[(WIN + 3) / 4 * 4 + 4];
    __shared__ uint32_t s_poison;                                  // one decision per workgroup
    const int ch = blockIdx.y, tid = threadIdx.x;
    const int o0 = blockIdx.x * ATILE;
    if (tid == 0) s_poison = poison_word(a.err);                   // read beside the staging loads
    const int m0 = D * o0 - 100;
    const bool last_tile = o0 + ATILE >= a.ny;
    // the last tile also computes up to the block end: stereo_dc's tail is the next block's history
    const int m1 = last_tile ? a.n : min(m0 + WIN, a.n);
    const float* fm = a.fm + (size_t)ch * a.fm_stride;
    const float* band = a.band + (size_t)ch * a.plain_stride;
    const float* tt = a.t + (size_t)ch * a.plain_stride;
    const float* sprev = a.sdc_prev + (size_t)ch * a.sdc_stride;
    float* scur = a.sdc + (size_t)ch * a.sdc_stride;
    const float car0 = a.car_prev[(size_t)ch * a.car_stride + a.n];
    // every load of the tile in flight at once (m1 <= m0 + WIN: the window of the last tile reaches
    // the block end), then the carriers, mixer products and LDS writes
    constexpr int NL = (WIN + AT - 1) / AT;
    float vb[NL], vt[NL], vf[NL];
#pragma unroll
    for (int u = 0; u < NL; u++) {
        const int i = m0 + tid + u * AT;
        const bool in = i < m1;
        vf[u] = in ? fm[i - 50] : 0.0f;                            // stereo.cpp:88
        vb[u] = (in && i >= 0) ? band[i] : (in ? sprev[a.n + i] : 0.0f);   // i >= -100: history
        vt[u] = (in && i > 0) ? tt[i - 1] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < NL; u++) {
        const int i = m0 + tid + u * AT, k = i - m0;
        if (i >= m1) continue;
        float sd = vb[u];
        if (i >= 0) {
            const float car = (i == 0) ? car0 : nco_carrier(vt[u], a.ncoScale, a.phaseAdjust);
            sd = (float)(2.0 * (double)vb[u] * (double)car);         // stereo.cpp:83-85
            if (i >= a.n - HIST) scur[i] = sd;
        }
        sb[k] = sd;
        sa[k] = vf[u];
    }
    if (last_tile && tid == 0) {                                   // carrier[n] (pll.cpp:52, :58)
        const float cl = nco_carrier(tt[a.n - 1], a.ncoScale, a.phaseAdjust);
        a.car[(size_t)ch * a.car_stride + a.n] = cl;
        a.st[ch].lastCarrier = cl;
    }
    __syncthreads();
    const int ob = o0 + tid * AR;
    if (ob >= a.ny) return;
    uint32_t* o = reinterpret_cast<uint32_t*>(a.lr + (size_t)ch * a.lr_stride) + ob;
    if (s_poison != 0u) {
        // a persistent PLL wait timed out (this block's phases were never computed, or not yet) or a
        // release wait did (the inputs may hold another block): the consumer gets a marked block
        // instead of audio (include/sdr_amd.h SDR_PCM_POISON)
        const uint32_t pp = (uint32_t)(uint16_t)SDR_PCM_POISON * 0x10001u;
#pragma unroll
        for (int r = 0; r < AR; r++)
            if (ob + r < a.ny) o[r] = pp;
        return;
    }
    const uint32_t late = poison_late(a.err);                      // after every input load of the tile
    float w[TW], m[AR], sv[AR];
    audio_window<D>(sa, tid, w);
    audio_mac<D>(a.h, w, m);                                       // mono resampler (:94)
    audio_window<D>(sb, tid, w);
    audio_mac<D>(a.h, w, sv);                                      // stereo resampler (:97)
    const bool bad = __builtin_amdgcn_readfirstlane(late) != 0u;
#pragma unroll
    for (int r = 0; r < AR; r++) {
        if (ob + r < a.ny) {
            const uint16_t l = (uint16_t)cvt_i16_x86(16384 * (m[r] + sv[r]));   // stereo.cpp:100-102
            const uint16_t rr = (uint16_t)cvt_i16_x86(16384 * (m[r] - sv[r]));
            o[r] = bad ? (uint32_t)(uint16_t)SDR_PCM_POISON * 0x10001u : (uint32_t)l | ((uint32_t)rr << 16);
        }
    }
}

// the unfused post stages' poison (SDR_FLAG_KEEP_INTERMEDIATES, the generic resamplers): rows
// [nch][n] of int16 overwritten with SDR_PCM_POISON when one of the block's error words is set
__global__ __launch_bounds__(BLK) void k_poison_i16(const Poison err, int16_t* __restrict__ p, size_t stride,
                                                    int n) {
    if (poison_word(err) == 0u) return;
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i < n) p[(size_t)blockIdx.y * stride + i] = SDR_PCM_POISON;
}

// ------------------------------------------------------------------------------------------
// RDS carrier and mixer in one pass (rds.cpp:119-127): ipll[i] from the 114 kHz PLL's phase
// (pll.cpp:52, ncoScale 0.5; ipll[0] = the previous block's last) and rds_dc[i] = (2 * delay[i]) *
// ipll[i] in f32 with delay[i] = rds_band[i - 50] + 0 (the APF of :122 is an exact 50-sample
// shift that turns -0 into +0) into the extended rds_dc stream, history included. ipll itself is
// not stored: only its last sample (the next block's ipll[0], and pllblock_args.lastCarrier).
// MIX_R samples per thread; the thread whose range holds n computes ipll[n].
// ------------------------------------------------------------------------------------------
struct RdsMix {
    const float* rband;         // this parity's rds_band, extended
    const float* t;             // PLL phases of this parity
    size_t fm_stride, plain_stride;
    float* car;                 // ipll rows of this parity: [ch][n] written
    const float* car_prev;      // the previous parity's: [ch][n] read
    size_t car_stride;
    sdr_pll_state* st;
    float ncoScale, phaseAdjust;
    float* rdc;                 // this parity's rds_dc, extended (history copied by tile 0)
    const float* rdc_prev;
    float* rfilt;               // this parity's rds_filt, extended: its history is copied by tile 0 too
    const float* rfilt_prev;
    size_t rf_stride;
    int n, n_rds;
};

// MIX_R consecutive samples per thread: one 16-byte load of the phases, two 8-byte loads of the
// delayed band (i - 50 = 2 mod 4), one 16-byte store -- 4x the bytes in flight per wave of the
// one-sample form, which waited on memory 74 % of its time (profiles/r03/stage_counters_v7.json)
constexpr int MIX_R = 4;
__global__ __launch_bounds__(BLK) void k_rds_mix(const RdsMix a) {
    const int ch = blockIdx.y;
    const int i0 = ((int)blockIdx.x * BLK + (int)threadIdx.x) * MIX_R;
    const float* tt = a.t + (size_t)ch * a.plain_stride;
    const float* rb = a.rband + (size_t)ch * a.fm_stride;
    float* y = a.rdc + (size_t)ch * a.fm_stride;
    auto carrier = [&](int i, float tprev) {
        return (i == 0) ? a.car_prev[(size_t)ch * a.car_stride + a.n] : nco_carrier(tprev, a.ncoScale, a.phaseAdjust);
    };
    if (i0 + MIX_R <= a.n) {
        const float4 tv = *reinterpret_cast<const float4*>(tt + i0);
        const float tm = i0 > 0 ? tt[i0 - 1] : 0.0f;
        const float2 r01 = *reinterpret_cast<const float2*>(rb + i0 - 50);
        const float2 r23 = *reinterpret_cast<const float2*>(rb + i0 - 48);
        const float tp[MIX_R] = {tm, tv.x, tv.y, tv.z};
        const float dl[MIX_R] = {r01.x, r01.y, r23.x, r23.y};
        float o[MIX_R];
#pragma unroll
        for (int k = 0; k < MIX_R; k++) {
            const float d = dl[k] + 0.0f;                                  // rds.cpp:122
            o[k] = 2 * d * carrier(i0 + k, tp[k]);                         // rds.cpp:125-127
        }
        *reinterpret_cast<float4*>(y + i0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        for (int k = 0; k < MIX_R; k++) {
            const int i = i0 + k;
            if (i < a.n) {
                const float d = rb[i - 50] + 0.0f;
                y[i] = 2 * d * carrier(i, i > 0 ? tt[i - 1] : 0.0f);
            } else if (i == a.n) {
                const float cl = nco_carrier(tt[a.n - 1], a.ncoScale, a.phaseAdjust);
                a.car[(size_t)ch * a.car_stride + a.n] = cl;
                a.st[ch].lastCarrier = cl;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < HIST) {
        y[(int)threadIdx.x - HIST] = a.rdc_prev[(size_t)ch * a.fm_stride + a.n - HIST + threadIdx.x];
        a.rfilt[(size_t)ch * a.rf_stride + (int)threadIdx.x - HIST] =
            a.rfilt_prev[(size_t)ch * a.rf_stride + a.n_rds - HIST + threadIdx.x];
    }
}

// ------------------------------------------------------------------------------------------
// The quadrature branch's carrier and mixer (SDR_FLAG_RDS_QUAD; no reference counterpart, the definition is
// at sdr_ctx_rds_clean_q in sdr_amd.h): k_rds_mix with phaseAdjust -pi/2 into streams of its own. It reads
// what k_rds_mix reads (rband, the PLL's phases) and writes no PLL state: ipll_q[n], the next block's
// ipll_q[0], goes to the row of this parity, and ipll_q[0] comes from the other parity's.
// ------------------------------------------------------------------------------------------
struct RdsMixQ {
    const float* rband;         // this parity's rds_band, extended
    const float* t;             // PLL phases of this parity
    size_t fm_stride, plain_stride;
    float* last;                // [nch] ipll_q[n] of this block
    const float* last_prev;     // [nch] the previous block's
    float ncoScale, phaseAdjust;
    float* rdc;                 // this parity's rds_dc_q, extended (history copied by tile 0)
    const float* rdc_prev;
    float* rfilt;               // this parity's rds_filt_q, extended: its history is copied by tile 0 too
    const float* rfilt_prev;
    size_t rf_stride;
    int n, n_rds;
};

__global__ __launch_bounds__(BLK) void k_rds_mix_q(const RdsMixQ a) {
    const int ch = blockIdx.y;
    const int i0 = ((int)blockIdx.x * BLK + (int)threadIdx.x) * MIX_R;
    const float* tt = a.t + (size_t)ch * a.plain_stride;
    const float* rb = a.rband + (size_t)ch * a.fm_stride;
    float* y = a.rdc + (size_t)ch * a.fm_stride;
    auto carrier = [&](int i, float tprev) {
        return (i == 0) ? a.last_prev[ch] : nco_carrier(tprev, a.ncoScale, a.phaseAdjust);
    };
    if (i0 + MIX_R <= a.n) {
        const float4 tv = *reinterpret_cast<const float4*>(tt + i0);
        const float tm = i0 > 0 ? tt[i0 - 1] : 0.0f;
        const float2 r01 = *reinterpret_cast<const float2*>(rb + i0 - 50);
        const float2 r23 = *reinterpret_cast<const float2*>(rb + i0 - 48);
        const float tp[MIX_R] = {tm, tv.x, tv.y, tv.z};
        const float dl[MIX_R] = {r01.x, r01.y, r23.x, r23.y};
        float o[MIX_R];
#pragma unroll
        for (int k = 0; k < MIX_R; k++) {
            const float d = dl[k] + 0.0f;
            o[k] = 2 * d * carrier(i0 + k, tp[k]);
        }
        *reinterpret_cast<float4*>(y + i0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        for (int k = 0; k < MIX_R; k++) {
            const int i = i0 + k;
            if (i < a.n) {
                const float d = rb[i - 50] + 0.0f;
                y[i] = 2 * d * carrier(i, i > 0 ? tt[i - 1] : 0.0f);
            } else if (i == a.n) {
                a.last[ch] = nco_carrier(tt[a.n - 1], a.ncoScale, a.phaseAdjust);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < HIST) {
        y[(int)threadIdx.x - HIST] = a.rdc_prev[(size_t)ch * a.fm_stride + a.n - HIST + threadIdx.x];
        a.rfilt[(size_t)ch * a.rf_stride + (int)threadIdx.x - HIST] =
            a.rfilt_prev[(size_t)ch * a.rf_stride + a.n_rds - HIST + threadIdx.x];
    }
}

// ------------------------------------------------------------------------------------------
// Mixers. stereo.cpp:83-85: stereo_dc = 2.0*band*carrier (f64 product, one rounding).
// rds.cpp:125-127: rds_dc = (2*delay)*ipll with delay[i] = rds_band[i-50] (the 101-tap APF of
// filter.cpp:73-78 is an exact 50-sample delay for finite inputs). Also copies the history.
// ------------------------------------------------------------------------------------------
template <bool RDS>
__global__ __launch_bounds__(BLK) void k_mix(const float* __restrict__ a, size_t a_stride,
                                             const float* __restrict__ c, size_t c_stride, int n,
                                             float* __restrict__ y, const float* __restrict__ y_other,
                                             size_t y_stride, int delay) {
    const int ch = blockIdx.y;
    const int i = blockIdx.x * BLK + threadIdx.x;
    const float* ac = a + (size_t)ch * a_stride;
    const float* cc = c + (size_t)ch * c_stride;
    float* yc = y + (size_t)ch * y_stride;
    if (i < n) {
        if (RDS) {
            const float d = ac[i - delay] + 0.0f;   // + 0.0f: the APF sum turns -0 into +0
            yc[i] = 2 * d * cc[i];
        } else {
            yc[i] = (float)(2.0 * (double)ac[i] * (double)cc[i]);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < HIST) {
        yc[(int)threadIdx.x - HIST] = y_other[(size_t)ch * y_stride + n - HIST + threadIdx.x];
    }
}

// copy the previous parity's last HIST samples in front of this parity's stream
__global__ void k_hist_copy(float* __restrict__ y, const float* __restrict__ y_other, size_t stride, int n) {
    const int ch = blockIdx.x;
    for (int i = threadIdx.x; i < HIST; i += blockDim.x)
        y[(size_t)ch * stride + i - HIST] = y_other[(size_t)ch * stride + n - HIST + i];
}

// Rows [nch][n] f32 from src to dst, and with hist_other the HIST samples in front of each dst row
// from the end of hist_other's row (the extended-stream history, as k_hist_copy): one pass at HBM
// rate (16-byte vectors when both rows are 16-byte aligned), where hipMemcpy2DAsync's rectangle blit
// moved the 30 MB of a 1024-channel fm_demod block at ~2 TB/s (31.8 us, profiles/r06/queue/).
constexpr int CR_BLK = 256, CR_V = 4;    // threads per workgroup, float4s per thread
__global__ __launch_bounds__(CR_BLK) void k_copy_rows(float* __restrict__ dst, size_t dst_stride,
                                                       const float* __restrict__ src, size_t src_stride, int n,
                                                       const float* __restrict__ hist_other, int vec) {
    const int ch = blockIdx.y;
    float* d = dst + (size_t)ch * dst_stride;
    const float* a = src + (size_t)ch * src_stride;
    if (hist_other && blockIdx.x == 0)
        for (int i = threadIdx.x; i < HIST; i += CR_BLK) d[i - HIST] = hist_other[(size_t)ch * dst_stride + n - HIST + i];
    const int i0 = blockIdx.x * CR_BLK * CR_V * 4;   // first float of this workgroup
    if (vec) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        f4* d4 = reinterpret_cast<f4*>(d + i0);
        const f4* a4 = reinterpret_cast<const f4*>(a + i0);
        f4 v[CR_V];
#pragma unroll
        for (int u = 0; u < CR_V; u++) {
            const int i = i0 + 4 * (threadIdx.x + u * CR_BLK);
            if (i + 3 < n) v[u] = __builtin_nontemporal_load(a4 + threadIdx.x + u * CR_BLK);
        }
#pragma unroll
        for (int u = 0; u < CR_V; u++) {
            const int i = i0 + 4 * (threadIdx.x + u * CR_BLK);
            if (i + 3 < n) d4[threadIdx.x + u * CR_BLK] = v[u];
            else for (int k = i; k < n && k < i + 4; k++) d[k] = a[k];
        }
    } else {
        for (int i = i0 + threadIdx.x; i < min(n, i0 + CR_BLK * CR_V * 4); i += CR_BLK) d[i] = a[i];
    }
}
int copy_rows(float* dst, size_t dst_stride, const float* src, size_t src_stride, int n, int nch,
              const float* hist_other, hipStream_t s) {
    const int vec = (reinterpret_cast<uintptr_t>(dst) % 16 == 0 && reinterpret_cast<uintptr_t>(src) % 16 == 0 &&
                     dst_stride % 4 == 0 && src_stride % 4 == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_copy_rows, dim3(cdiv(n, CR_BLK * CR_V * 4), nch), dim3(CR_BLK), 0, s, dst, dst_stride, src,
                       src_stride, n, hist_other, vec);
    LAUNCH_CHECK();
    return SDR_OK;
}

// RDS symbol and bit recovery for one block (rds.cpp:135-167): cdr, slicer (:157-161),
// manchester_decode (rds_utilities.cpp:34-68), differential_decode (:70-88).
// dec[ch*8 + {0..4}] = block_count, half_symbol, start, last_bit, sample_offset.
__global__ __launch_bounds__(64) void k_rds_bits(const float* __restrict__ x, size_t x_stride, int n, int sps,
                                                 int rds_on, int32_t* __restrict__ dec,
                                                 int32_t* __restrict__ offset_out, int32_t* __restrict__ nsym_out,
                                                 uint8_t* __restrict__ sym_out, size_t sym_stride,
                                                 int32_t* __restrict__ nbits_out, uint8_t* __restrict__ bits_out,
                                                 size_t bits_stride, const Poison err, int vec4) {
    // dynamic LDS: the channel's whole block (n floats), staged with every load in flight (the cdr
    // reads it 39-strided and the slicer sps-strided: from LDS, not global memory)
    extern __shared__ float4 xs4[];
    float* xs = reinterpret_cast<float*>(xs4);
    __shared__ uint8_t symbols[SDR_MAX_SYMS];
    const int ch = blockIdx.x;
    const int lane = threadIdx.x;
    int32_t* d = dec + (size_t)ch * DEC_STATE;
    const int block_count = d[0];
    const float* xc = x + (size_t)ch * x_stride;
    const bool decode = (block_count > 5) && rds_on;
    if (poison_word(err) != 0u) {   // a persistent PLL or release wait timed out: no bits from this block
        if (lane == 0) {
            if (offset_out) offset_out[ch] = -1;
            if (nsym_out) nsym_out[ch] = 0;
            if (nbits_out) nbits_out[ch] = SDR_NBITS_POISONED;
        }
        return;
    }
    if (!decode) {
        if (lane == 0) {
            if (offset_out) offset_out[ch] = d[4];
            if (nsym_out) nsym_out[ch] = 0;
            if (nbits_out) nbits_out[ch] = -1;
            d[0] = block_count + 1;
        }
        return;
    }
    {
        // the whole row in one round of loads where it fits: 16-byte loads when the row is aligned
        // (VEC4), then the LDS writes
        constexpr int U4 = 12;
        int i_tail = 0;
        if (vec4) {
            const int n4 = n >> 2;
            for (int q0 = lane; q0 < n4; q0 += 64 * U4) {
                // loads and LDS writes unconditional at a clamped index (lanes past the row rewrite its
                // last element with the same value): conditional ones went to scratch, or were sunk
                // next to their writes, one load in flight at a time
                float4 v[U4];
#pragma unroll
                for (int u = 0; u < U4; u++) v[u] = reinterpret_cast<const float4*>(xc)[min(q0 + 64 * u, n4 - 1)];
#pragma unroll
                for (int u = 0; u < U4; u++) reinterpret_cast<float4*>(xs)[min(q0 + 64 * u, n4 - 1)] = v[u];
            }
            i_tail = n4 * 4;
        }
        constexpr int U = 8;
        for (int i0 = i_tail + lane; i0 < n; i0 += 64 * U) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; u++) v[u] = (i0 + 64 * u < n) ? xc[i0 + 64 * u] : 0.0f;
#pragma unroll
            for (int u = 0; u < U; u++)
                if (i0 + 64 * u < n) xs[i0 + 64 * u] = v[u];
        }
        __syncthreads();
    }
    const int off = cdr_wave(xs, n, sps);
    int m = 0;
    if (off < n) m = (n - off + sps - 1) / sps;     // i with off + i*sps < n
    if (m > SDR_MAX_SYMS) m = SDR_MAX_SYMS;
    for (int i = lane; i < m; i += 64) symbols[i] = xs[off + i * sps] > 0;
    __syncthreads();
    // manchester_decode + differential_decode with every lane: bit k of the block is half_symbol
    // (k < nb0, a symbol pair split across blocks) or symbols[start + 2 (k - nb0)]; the outputs are
    // bits[k] ^ bits[k-1] (bits[-1] = the previous block's last bit), the state comes from the ends
    const int half_in = d[1], start_in = d[2], last_in = d[3];
    const int nb0 = start_in ? 1 : 0;
    int start = start_in;
    if (block_count == 0) {  // dead in the reference (decoding starts at block 6), kept for parity
        int score = 0;
        for (int i = 0; i < m - 1; i += 2) score += symbols[i] ^ symbols[i + 1];
        for (int j = 1; j < m - 1; j += 2) score -= symbols[j] ^ symbols[j + 1];
        start = score < 0;
    }
    const int npairs = m - 1 > start ? (m - start) / 2 : 0;       // i = start, start + 2, ... < m - 1
    const int nb = min(nb0 + npairs, SDR_MAX_BITS);
    auto bit_at = [&](int k) -> int { return k < nb0 ? half_in : symbols[start + 2 * (k - nb0)]; };
    uint8_t* bo = bits_out ? bits_out + (size_t)ch * bits_stride : nullptr;
    if (bo) {
        for (int k = lane; k < nb; k += 64) {
            const int prev = k == 0 ? (block_count == 0 ? 0 : last_in) : bit_at(k - 1);
            bo[k] = (uint8_t)(bit_at(k) ^ prev);
        }
    }
    if (sym_out) {
        uint8_t* so = sym_out + (size_t)ch * sym_stride;
        for (int i = lane; i < m; i += 64) so[i] = symbols[i];
    }
    if (lane == 0) {
        const bool odd = ((m - start) & 0x01) == 1;
        d[1] = odd ? symbols[m - 1] : half_in;
        d[2] = odd ? 1 : 0;
        d[3] = nb > 0 ? bit_at(nb - 1) : last_in;
        d[4] = off;
        d[0] = block_count + 1;
        if (offset_out) offset_out[ch] = off;
        if (nsym_out) nsym_out[ch] = m;
        if (nbits_out) nbits_out[ch] = nb;
    }
}

// the error words of the current block's output stages (kernel side: Poison)
Poison block_poison(const sdr_ctx* c) { return Poison{c->pers.err(c->block), c->rel.fail_words}; }

int check_iq(const sdr_ctx* c, const uint8_t* iq, size_t iq_stride) {
    const sdr_info& in = c->info;
    if (iq_stride < (size_t)2 * in.block_iq || (iq_stride & 1) || (reinterpret_cast<uintptr_t>(iq) & 1))
        return fail(SDR_E_INVALID, "iq_stride %zu < 2*block_iq %d or misaligned", iq_stride, 2 * in.block_iq);
    return SDR_OK;
}

// the timed launches' earliest workgroup start and latest workgroup end (100 MHz ticks)
int frontend_spans(sdr_ctx* c, int k, unsigned long long* t0, unsigned long long* t1) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t per = (size_t)c->fe_time.stamp_wgs * 2;
    std::vector<unsigned long long> h(per);
    for (int i = 0; i < k; i++) {
        HIP_TRY(hipMemcpy(h.data(), c->fe_time.stamps + (size_t)i * per, per * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost));
        unsigned long long lo = ~0ull, hi = 0;
        for (size_t g = 0; g < per; g += 2) {
            lo = std::min(lo, h[g]);
            hi = std::max(hi, h[g + 1]);
        }
        t0[i] = lo;
        t1[i] = hi;
    }
    return SDR_OK;
}

// launch k_fir_rb with NT tap sets (one block of every channel of length n)
// tiles [x0, x0 + xn) of the block (xn <= 0: all)
template <int NT, bool SQUARE>
int fir_rb(const sdr_ctx* c, const float* x, size_t x_stride, int n, FirRb f, hipStream_t s, int x0 = 0,
           int xn = 0) {
    if (xn <= 0) { x0 = 0; xn = cdiv(n, FRB_TILE); }
    f.x0 = x0;
    // the 2- and 3-set passes with their first two sets (pilot, band) as packed pairs
    if constexpr (NT >= 2 && !SQUARE) {
        if (f.h01) {
            hipLaunchKernelGGL((k_fir_rb<NT, false, true>), dim3(xn, c->nch), dim3(BLK), 0, s, x,
                               x_stride, x, x_stride, n, f);
            LAUNCH_CHECK();
            return SDR_OK;
        }
    }
    hipLaunchKernelGGL((k_fir_rb<NT, SQUARE>), dim3(xn, c->nch), dim3(BLK), 0, s, x, x_stride, x,
                       x_stride, n, f);
    LAUNCH_CHECK();
    return SDR_OK;
}
// pilot BPF (stereo.cpp:74) -> pilot + its PLL reciprocals, band BPF (:80) -> band
FirRb stereo_fir(sdr_ctx* c) {
    FirRb f{};
    f.h[0] = c->pilot_h;
    f.h[1] = c->stereo_h;
    f.y[0] = c->plain(c->pilot);
    f.y[1] = c->plain(c->band);
    f.y_stride[0] = f.y_stride[1] = c->plain_stride;
    f.rx0 = c->rxbuf(c->rx_st);
    f.rx_stride = c->plain_stride;
    f.y0neg = c->plain(c->pilot_neg);
    // (not as the packed pair of the 3-set pass: k_fir_rb<2, false, true> measured 133 against 120 us
    // for the scalar 2-set pass, profiles/r06/queue/)
    return f;
}
// squaring (rds.cpp:111-113) + 114 kHz BPF (:116) of the extended rds_band stream -> gen_pilot + its
// PLL reciprocals
int rds_sq_fir(sdr_ctx* c, hipStream_t s, int x0 = 0, int xn = 0) {
    FirRb f{};
    f.h[0] = c->rds_sq_h;
    f.y[0] = c->plain(c->gpilot);
    f.y_stride[0] = c->plain_stride;
    f.rx0 = c->rxbuf(c->rx_rds);
    f.rx_stride = c->plain_stride;
    f.y0neg = c->plain(c->gpilot_neg);
    return fir_rb<1, true>(c, c->rband + c->parity * c->fm_par, c->fm_stride, c->info.block_if, f, s, x0, xn);
}

// pilot, band and RDS band BPFs (stereo.cpp:74,80, rds.cpp:105) from one staged fm_demod window --
// the third output into the extended rds_band stream, history included -- then the squared 114 kHz
// BPF; FIR tiles [x0, x0 + xn) of the block (xn <= 0: all)
int pre_launch(sdr_ctx* c, hipStream_t s, int x0 = 0, int xn = 0) {
    const int n = c->info.block_if, p = c->parity;
    FirRb f = stereo_fir(c);
    f.h[2] = c->rds_h;
    f.h01 = c->pilot_band_h;
    f.y[2] = c->rband + p * c->fm_par;
    f.y_stride[2] = c->fm_stride;
    f.hist2_src = c->rband + (p ^ 1) * c->fm_par;
    const int r = fir_rb<3, false>(c, c->fm_cur(), c->fm_stride, n, f, s, x0, xn);
    return r ? r : rds_sq_fir(c, s, x0, xn);
}

}  // namespace

extern "C" {

int sdr_frontend(sdr_ctx* c, const uint8_t* iq, size_t iq_stride, void* stream) {
    if (!c || !iq) return fail(SDR_E_INVALID, "null argument");
    if (const int rf_ = check_failed(c, "frontend")) return rf_;
    if (const int r = check_iq(c, iq, iq_stride)) return r;
    if (c->tn_nsrc > 0) return fail(SDR_E_INVALID, "frontend: the context is tuned (sdr_frontend_tuned)");
    const int p = c->parity ^ 1;
    // fm of parity p, and the pre stages' buffers too (one wait kernel: sdr_pre on this stream then
    // has nothing left to wait for; waiting for the RDS mixer only before the pre stages measured the
    // same, profiles/r04/release/)
    if (const int rw = release_wait(c, p, REL_ALL, S(stream))) return rw;
    FrontendArgs a = frontend_args(c, iq, iq_stride, p);
    sdr_ctx::FeTime& ft = c->fe_time;
    const bool timed = ft.n < ft.cap;
    if (timed && ft.use_stamps) {      // sdr_frontend_timing: the kernel's own workgroup stamps
        a.stamps = ft.stamps + (size_t)ft.n * ft.stamp_wgs * 2;
    } else if (timed) {                // (other front ends) HIP events recorded with the launch
        a.ev0 = ft.ev[2 * ft.n];
        a.ev1 = ft.ev[2 * ft.n + 1];
    }
    const int r = frontend_launch(a, S(stream));
    if (r) return r;
    if (timed) ft.n++;
    c->parity = p;
    c->block++;
    if (a.env) c->env_block = c->block;
    return SDR_OK;
}

// ---- shared-capture tuner: channel ch = source row src[ch] shifted by khz[ch] kHz (sdr_frontend.hip)
// the rule for a tuning of nch channels at N = rf_Fs / 1000 (nsrc = 0: untuned); `who` names the caller in the text
static int tuner_rule(const char* who, int N, int nch, int nsrc, const int32_t* src, const int32_t* khz) {
    if (nsrc < 0 || nsrc > nch) return fail(SDR_E_INVALID, "%s: nsrc %d outside [0, nch %d]", who, nsrc, nch);
    if (nsrc == 0) return SDR_OK;
    if (!src || !khz) return fail(SDR_E_INVALID, "%s: null src or khz", who);
    for (int ch = 0; ch < nch; ch++) {
        if (src[ch] < 0 || src[ch] >= nsrc)
            return fail(SDR_E_INVALID, "%s: src[%d] = %d outside [0, %d)", who, ch, (int)src[ch], nsrc);
        if (2 * (long long)khz[ch] <= -(long long)N || 2 * (long long)khz[ch] > N)
            return fail(SDR_E_INVALID, "%s: khz[%d] = %d outside (-%d/2, %d/2]", who, ch, (int)khz[ch], N, N);
    }
    return SDR_OK;
}

int sdr_tuner_check(int mode, int nch, int nsrc, const int32_t* src, const int32_t* khz) {
    sdr_info in;
    if (const int r = mode_info(&in, nch, mode, 1)) return r;
    return tuner_rule("tuner_check", in.rf_Fs / 1000, nch, nsrc, src, khz);
}

int sdr_tuner_set(sdr_ctx* c, int nsrc, const int32_t* src, const int32_t* khz, void* stream) {
    if (!c) return fail(SDR_E_INVALID, "tuner_set: null context");
    if (c->block != -1) return fail(SDR_E_INVALID, "tuner_set: only at block 0 (after create or sdr_ctx_reset)");
    if (!c->tn_tab) return fail(SDR_E_INVALID, "tuner_set: the context has no tuned front end");
    const int N = c->info.rf_Fs / 1000;
    if (const int r = tuner_rule("tuner_set", N, c->nch, nsrc, src, khz)) return r;
    c->fe_time.cap = c->fe_time.n = 0;   // (the timed launches' stamp layout belongs to the other kernel)
    if (nsrc == 0) {
        c->tn_nsrc = 0;
        return SDR_OK;
    }
    // grid order: channels sorted by source row (stable), so the stations of a row are neighbours;
    // the first of each row stores the row's tail
    std::vector<int> ord(c->nch);
    for (int ch = 0; ch < c->nch; ch++) ord[ch] = ch;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return src[a] < src[b]; });
    std::vector<int32_t> tab((size_t)4 * c->nch);
    for (int pos = 0; pos < c->nch; pos++) {
        const int ch = ord[pos];
        tab[4 * pos + 0] = ch;
        tab[4 * pos + 1] = src[ch];
        tab[4 * pos + 2] = ((khz[ch] % N) + N) % N;
        tab[4 * pos + 3] = (pos == 0 || src[ord[pos - 1]] != src[ch]) ? 1 : 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->tn_tab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));   // (tab is a local)
    c->tn_nsrc = nsrc;
    return SDR_OK;
}

int sdr_tuner_get(const sdr_ctx* c, int* nsrc) {
    if (!c || !nsrc) return fail(SDR_E_INVALID, "tuner_get: null argument");
    *nsrc = c->tn_nsrc;
    return SDR_OK;
}

int sdr_frontend_tuned(sdr_ctx* c, const uint8_t* iq, size_t iq_stride, void* stream) {
    if (!c || !iq) return fail(SDR_E_INVALID, "null argument");
    if (const int rf_ = check_failed(c, "frontend_tuned")) return rf_;
    if (const int r = check_iq(c, iq, iq_stride)) return r;
    if (c->tn_nsrc <= 0) return fail(SDR_E_INVALID, "frontend_tuned: the context is not tuned (sdr_tuner_set)");
    const int p = c->parity ^ 1;
    if (const int rw = release_wait(c, p, REL_ALL, S(stream))) return rw;
    FrontendArgs a = frontend_args(c, iq, iq_stride, p);   // (the tail rows are per source row here)
    sdr_ctx::FeTime& ft = c->fe_time;
    const bool timed = ft.n < ft.cap && ft.use_stamps &&
                       ft.stamp_wgs == frontend_tuned_wgs(c->info.block_if, c->nch, c->nxcc);
    if (timed) a.stamps = ft.stamps + (size_t)ft.n * ft.stamp_wgs * 2;
    // the block being produced is c->block + 1: its first sample is sample (block * block_iq) of the stream
    const long long N = c->info.rf_Fs / 1000;
    const int phase0 = (int)((((c->block + 1) % N) * (c->info.block_iq % N)) % N);
    const int r = frontend_tuned_launch(a, c->rf_ht, c->tn_q, c->tn_tab, phase0, c->nxcc, S(stream));
    if (r) return r;
    if (timed) ft.n++;
    c->parity = p;
    c->block++;
    if (a.env) c->env_block = c->block;
    return SDR_OK;
}

int sdr_frontend_timing(sdr_ctx* c, int max_launches) {
    if (!c || max_launches < 0) return fail(SDR_E_INVALID, "frontend_timing: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    const sdr_info& in = c->info;
    const int wgs = c->tn_nsrc > 0 ? frontend_tuned_wgs(in.block_if, c->nch, c->nxcc)
                                   : frontend_stamp_wgs(in.block_if, c->nch, c->ntaps, in.rf_decim,
                                                        c->flags & SDR_FLAG_FAST_FRONTEND);
    sdr_ctx::FeTime& ft = c->fe_time;
    ft.use_stamps = wgs > 0;
    if (ft.use_stamps) {
        if (ft.stamp_cap < max_launches || ft.stamp_wgs != wgs) {
            if (ft.stamps) {
                HIP_TRY(hipDeviceSynchronize());   // a pending timed launch may still write the old buffer
                HIP_TRY(hipFree(ft.stamps));
                ft.stamps = nullptr;
            }
            void* p = nullptr;
            HIP_TRY(hipMalloc(&p, (size_t)std::max(max_launches, 1) * wgs * 2 * sizeof(unsigned long long)));
            ft.stamps = static_cast<unsigned long long*>(p);
            ft.stamp_cap = max_launches;
            ft.stamp_wgs = wgs;
        }
    } else {
        while ((int)ft.ev.size() < 2 * max_launches) {
            hipEvent_t e = nullptr;
            HIP_TRY(hipEventCreate(&e));
            ft.ev.push_back(e);
        }
    }
    ft.cap = max_launches;
    ft.n = 0;
    return SDR_OK;
}

int sdr_frontend_stamps(sdr_ctx* c, unsigned long long* t_start, unsigned long long* t_end, int max, int* n) {
    if (!c || !t_start || !t_end || max < 0) return fail(SDR_E_INVALID, "frontend_stamps: bad arguments");
    if (!c->fe_time.use_stamps) return fail(SDR_E_INVALID, "frontend_stamps: only the 101-tap front ends stamp themselves");
    const int k = std::min(c->fe_time.n, max);
    if (const int r = frontend_spans(c, k, t_start, t_end)) return r;
    if (n) *n = k;
    return SDR_OK;
}

int sdr_frontend_times(sdr_ctx* c, double* ms, int max, int* n) {
    if (!c || (!ms && max > 0)) return fail(SDR_E_INVALID, "frontend_times: bad arguments");
    const sdr_ctx::FeTime& ft = c->fe_time;
    const int k = std::min(ft.n, std::max(max, 0));
    if (ft.use_stamps) {
        // each launch: the earliest workgroup start to the latest workgroup end
        std::vector<unsigned long long> t0((size_t)std::max(k, 1)), t1((size_t)std::max(k, 1));
        if (const int r = frontend_spans(c, k, t0.data(), t1.data())) return r;
        for (int i = 0; i < k; i++) ms[i] = t1[i] >= t0[i] ? (double)(t1[i] - t0[i]) * 1e-5 : -1.0;
    } else {
        if (k > 0) HIP_TRY(hipEventSynchronize(ft.ev[2 * ft.n - 1]));
        for (int i = 0; i < k; i++) {
            float t = 0.0f;
            HIP_TRY(hipEventElapsedTime(&t, ft.ev[2 * i], ft.ev[2 * i + 1]));
            ms[i] = t;
        }
    }
    if (n) *n = k;
    return SDR_OK;
}

int sdr_frontend_release_wait(sdr_ctx* c, void* stream) {
    if (!c) return fail(SDR_E_INVALID, "null context");
    if (const int rf_ = check_failed(c, "frontend_release_wait")) return rf_;
    // the wait the next sdr_frontend (or sdr_frontend_pre_parts) enqueues first; it then finds the
    // counts already waited for on this stream and enqueues none
    return release_wait(c, c->parity ^ 1, REL_ALL, S(stream));
}

int sdr_get_fm_demod(sdr_ctx* c, float* fm, size_t fm_stride, void* stream) {
    if (!c || !fm) return fail(SDR_E_INVALID, "null argument");
    if (const int rf_ = check_failed(c, "get_fm_demod")) return rf_;
    if (c->block < 0) return fail(SDR_E_INVALID, "no block processed yet");
    const sdr_info& in = c->info;
    return copy_rows(fm, fm_stride, c->fm_cur(), c->fm_stride, in.block_if, c->nch, nullptr, S(stream));
}

int sdr_mono(sdr_ctx* c, int16_t* audio, size_t audio_stride, void* stream) {
    if (!c || !audio) return fail(SDR_E_INVALID, "null argument");
    if (const int rf_ = check_failed(c, "mono")) return rf_;
    if (c->block < 0 || c->mono_done == c->block) return fail(SDR_E_INVALID, "mono: no new block");
    const sdr_info& in = c->info;
    const float* fm = c->fm_cur();
    if (c->audio_u1_101 && (in.audio_decim == 5 || in.audio_decim == 9)) {   // register-blocked, modes 0 and 1
        const dim3 g(cdiv(in.n_audio, ATILE), c->nch);
        if (in.audio_decim == 5)
            hipLaunchKernelGGL(k_mono_out<5>, g, dim3(AT), 0, S(stream), fm, c->fm_stride, c->audio_pp, in.block_if,
                               in.n_audio, audio, audio_stride, block_poison(c));
        else
            hipLaunchKernelGGL(k_mono_out<9>, g, dim3(AT), 0, S(stream), fm, c->fm_stride, c->audio_pp, in.block_if,
                               in.n_audio, audio, audio_stride, block_poison(c));
        LAUNCH_CHECK();
        c->mono_done = c->block;
        if (const int r = pers_reader_mark(c, S(stream))) return r;
        return release_record(c, REL_MONO, S(stream));
    }
    const int tile = 512;
    dim3 grid(cdiv(in.n_audio, tile), c->nch);
    const size_t lds = resample_lds_bytes(c->audio_L, in.audio_upsample, in.audio_decim, tile, 1);
    auto km = c->audio_u1_101 ? k_resample<1, 101> : k_resample<1, 0>;
    hipLaunchKernelGGL(km, grid, dim3(BLK), lds, S(stream), fm, fm, c->fm_stride, c->fm_stride,
                       nullptr, nullptr, (size_t)0, (size_t)0, c->audio_pp, c->audio_cnt, c->audio_L,
                       in.audio_upsample, in.audio_decim, in.n_audio, tile, -HIST, (void*)audio, audio_stride);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_poison_i16, dim3(cdiv(in.n_audio, BLK), c->nch), dim3(BLK), 0, S(stream), block_poison(c),
                       audio, audio_stride, in.n_audio);
    LAUNCH_CHECK();
    c->mono_done = c->block;
    if (const int r = pers_reader_mark(c, S(stream))) return r;
    return release_record(c, REL_MONO, S(stream));
}

// The stereo and RDS loop bodies split at their PLL (pre: FIRs feeding the PLL; pll: the serial
// recurrence; post: everything after it), so a caller can run the PLL of block b on its own stream
// back to back with block b+1's while other streams do the rest. Intermediates that cross the
// split are kept per block parity. sdr_stereo / sdr_rds_dsp run the three parts on one stream.
int sdr_stereo_pre(sdr_ctx* c, void* stream) {
    if (!c) return fail(SDR_E_INVALID, "null context");
    if (const int rf_ = check_failed(c, "stereo_pre")) return rf_;
    if (c->block < 0 || c->st_pre_done == c->block) return fail(SDR_E_INVALID, "stereo_pre: no new block");
    if (c->ntaps != FRB_T) return fail(SDR_E_INVALID, "stereo_pre: %d taps", c->ntaps);
    // band of this parity read by the stereo post stage two blocks back (pilot by the meter)
    if (const int rw = release_wait(c, c->parity, REL_STEREO | REL_METER_A, S(stream))) return rw;
    // pilot BPF (stereo.cpp:74) + band BPF (:80) from one staged window of fm_demod
    const int r = fir_rb<2, false>(c, c->fm_cur(), c->fm_stride, c->info.block_if, stereo_fir(c), S(stream));
    if (r) return r;
    c->st_pre_done = c->block;
    return SDR_OK;
}

int sdr_stereo_pll(sdr_ctx* c, void* stream) {
    if (!c) return fail(SDR_E_INVALID, "null context");
    if (const int rf_ = check_failed(c, "stereo_pll")) return rf_;
    if (c->st_pre_done != c->block || c->st_pll_done == c->block)
        return fail(SDR_E_INVALID, "stereo_pll: run sdr_stereo_pre on a new block first");
    PllJobs jobs{};
    jobs.j[0] = stereo_job(c);   // PLL 19 kHz -> 38 kHz carrier (stereo.cpp:77); NCO output: stereo_post
    const int r = launch_plls(c->flags & SDR_FLAG_PLL_LIBM, jobs, 1, c->info.block_if, c->nch, S(stream), false);
    if (r) return r;
    c->st_pll_done = c->block;
    return SDR_OK;
}

int sdr_stereo_post(sdr_ctx* c, int16_t* lr, size_t lr_stride, void* stream) {
    if (!c || !lr) return fail(SDR_E_INVALID, "null argument");
    if (const int rf_ = check_failed(c, "stereo_post")) return rf_;
    if (c->st_pll_done != c->block || c->stereo_done == c->block)
        return fail(SDR_E_INVALID, "stereo_post: run sdr_stereo_pll on a new block first");
    if (const int rf = check_pers_failed(c, "stereo_post")) return rf;
    const sdr_info& in = c->info;
    hipStream_t s = S(stream);
    const int n = in.block_if;
    const float* fm = c->fm_cur();
    if (!(c->flags & SDR_FLAG_KEEP_INTERMEDIATES) && c->audio_u1_101 &&
        (in.audio_decim == 5 || in.audio_decim == 9)) {
        // NCO, mixer, mono delay, both resamplers and L/R in one pass (k_stereo_out)
        const int p = c->parity;
        StereoOut a{};
        a.fm = fm;
        a.band = c->plain(c->band);
        a.t = c->plain(c->t_st);
        a.fm_stride = c->fm_stride;
        a.plain_stride = c->plain_stride;
        a.car = c->pllbuf(c->carrier);
        a.car_prev = c->carrier + (p ^ 1) * c->pll_par;
        a.car_stride = c->pll_stride;
        a.st = c->st_pll;
        a.ncoScale = 2.0f;                          // stereo.cpp:77: fmpll(..., 2.0, 0, 0.01)
        a.phaseAdjust = 0.0f;
        a.sdc = c->sdc + p * c->fm_par;
        a.sdc_prev = c->sdc + (p ^ 1) * c->fm_par;
        a.sdc_stride = c->fm_stride;
        a.h = c->audio_pp;
        a.n = n;
        a.ny = in.n_audio;
        a.lr = lr;
        a.lr_stride = lr_stride;
        a.err = block_poison(c);
        const dim3 g(cdiv(in.n_audio, ATILE), c->nch);
        if (in.audio_decim == 5)
            hipLaunchKernelGGL(k_stereo_out<5>, g, dim3(AT), 0, s, a);
        else
            hipLaunchKernelGGL(k_stereo_out<9>, g, dim3(AT), 0, s, a);
        LAUNCH_CHECK();
        c->stereo_done = c->block;
        if (const int r = pers_reader_mark(c, s)) return r;
        return release_record(c, REL_STEREO, s);
    }
    {
        // NCO output of this block's PLL phases (pll.cpp:52), carrier[0] = last of the previous block
        PllJobs jobs{};
        jobs.j[0] = stereo_job(c);
        const int r = launch_nco(jobs, 1, n, c->nch, s);
        if (r) return r;
    }
    // mixer (stereo.cpp:83-85) into the extended stereo_dc stream
    const int p = c->parity;
    float* sdc = c->sdc + p * c->fm_par;
    hipLaunchKernelGGL(k_mix<false>, dim3(cdiv(n, BLK), c->nch), dim3(BLK), 0, s, c->plain(c->band),
                       c->plain_stride, c->pllbuf(c->carrier), c->pll_stride, n, sdc, c->sdc + (p ^ 1) * c->fm_par,
                       c->fm_stride, 0);
    LAUNCH_CHECK();
    // mono delay (:88, exact 50-sample shift of fm_demod) + both resamplers + L/R (:94-107)
    const int tile = 512;
    dim3 gr(cdiv(in.n_audio, tile), c->nch);
    const size_t lds = resample_lds_bytes(c->audio_L, in.audio_upsample, in.audio_decim, tile, 2);
    auto ks = c->audio_u1_101 ? k_resample<2, 101> : k_resample<2, 0>;
    hipLaunchKernelGGL(ks, gr, dim3(BLK), lds, s, fm - 50, fm - 50, c->fm_stride, c->fm_stride, sdc, sdc,
                       c->fm_stride, c->fm_stride, c->audio_pp, c->audio_cnt, c->audio_L, in.audio_upsample,
                       in.audio_decim, in.n_audio, tile, -(HIST - 50), (void*)lr, lr_stride);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_poison_i16, dim3(cdiv(2 * in.n_audio, BLK), c->nch), dim3(BLK), 0, s, block_poison(c), lr,
                       lr_stride, 2 * in.n_audio);
    LAUNCH_CHECK();
    c->stereo_done = c->block;
    if (const int r = pers_reader_mark(c, s)) return r;
    return release_record(c, REL_STEREO, s);
}

int sdr_stereo(sdr_ctx* c, int16_t* lr, size_t lr_stride, void* stream) {
    if (!c || !lr) return fail(SDR_E_INVALID, "null argument");
    if (c->block < 0 || c->stereo_done == c->block) return fail(SDR_E_INVALID, "stereo: no new block");
    int r = sdr_stereo_pre(c, stream);
    if (!r) r = sdr_stereo_pll(c, stream);
    if (!r) r = sdr_stereo_post(c, lr, lr_stride, stream);
    return r;
}

int sdr_rds_pre(sdr_ctx* c, void* stream) {
    if (!c) return fail(SDR_E_INVALID, "null context");
    if (const int rf_ = check_failed(c, "rds_pre")) return rf_;
    if (c->block < 0 || c->rds_pre_done == c->block) return fail(SDR_E_INVALID, "rds_pre: no new block");
    if (c->ntaps != FRB_T) return fail(SDR_E_INVALID, "rds_pre: %d taps", c->ntaps);
    hipStream_t s = S(stream);
    const int n = c->info.block_if, p = c->parity;
    float* rband = c->rband + p * c->fm_par;
    if (const int rw = release_wait(c, p, REL_RDS | REL_METER_R, s)) return rw;   // rband read by the RDS mixer (and the meter)
    // RDS band BPF (rds.cpp:105) into the extended rds_band stream
    hipLaunchKernelGGL(k_hist_copy, dim3(c->nch), dim3(HIST), 0, s, rband, c->rband + (p ^ 1) * c->fm_par,
                       c->fm_stride, n);
    LAUNCH_CHECK();
    FirRb f{};
    f.h[0] = c->rds_h;
    f.y[0] = rband;
    f.y_stride[0] = c->fm_stride;
    int r = fir_rb<1, false>(c, c->fm_cur(), c->fm_stride, n, f, s);
    if (!r) r = rds_sq_fir(c, s);
    if (r) return r;
    c->rds_pre_done = c->block;
    return SDR_OK;
}

int sdr_pre(sdr_ctx* c, void* stream) {
    if (!c) return fail(SDR_E_INVALID, "null context");
    if (const int rf_ = check_failed(c, "pre")) return rf_;
    if (c->block < 0 || c->st_pre_done == c->block || c->rds_pre_done == c->block)
        return fail(SDR_E_INVALID, "pre: no new block");
    if (!c->rds_on) return sdr_stereo_pre(c, stream);
    if (c->ntaps != FRB_T) return fail(SDR_E_INVALID, "pre: %d taps", c->ntaps);
    if (const int rw = release_wait(c, c->parity, REL_STEREO | REL_RDS | REL_METER_A | REL_METER_R, S(stream))) return rw;
    const int r = pre_launch(c, S(stream));
    if (r) return r;
    c->st_pre_done = c->rds_pre_done = c->block;
    return SDR_OK;
}

int sdr_rds_pll(sdr_ctx* c, void* stream) {
    if (!c) return fail(SDR_E_INVALID, "null context");
    if (const int rf_ = check_failed(c, "rds_pll")) return rf_;
    if (c->rds_pre_done != c->block || c->rds_pll_done == c->block)
        return fail(SDR_E_INVALID, "rds_pll: run sdr_rds_pre on a new block first");
    PllJobs jobs{};
    jobs.j[0] = rds_job(c);      // PLL 114 kHz -> 57 kHz (rds.cpp:119); NCO output: rds_post
    const int r = launch_plls(c->flags & SDR_FLAG_PLL_LIBM, jobs, 1, c->info.block_if, c->nch, S(stream), false);
    if (r) return r;
    c->rds_pll_done = c->block;
    return SDR_OK;
}

int sdr_plls(sdr_ctx* c, void* stream) {
    if (!c) return fail(SDR_E_INVALID, "null context");
    if (const int rf_ = check_failed(c, "plls")) return rf_;
    if (c->st_pre_done != c->block || c->st_pll_done == c->block || c->rds_pre_done != c->block ||
        c->rds_pll_done == c->block)
        return fail(SDR_E_INVALID, "plls: run sdr_stereo_pre and sdr_rds_pre on a new block first");
    PllJobs jobs{};
    jobs.j[0] = stereo_job(c);
    jobs.j[1] = rds_job(c);
    const int r = launch_plls(c->flags & SDR_FLAG_PLL_LIBM, jobs, 2, c->info.block_if, c->nch, S(stream), false);
    if (r) return r;
    c->st_pll_done = c->rds_pll_done = c->block;
    return SDR_OK;
}

int sdr_frontend_pre_parts(sdr_ctx* c, const uint8_t* iq, size_t iq_stride, int nparts, void* stream) {
    if (!c || !iq || nparts < 1) return fail(SDR_E_INVALID, "frontend_pre_parts: bad arguments");
    if (const int rf_ = check_failed(c, "frontend_pre_parts")) return rf_;
    if (const int r = check_iq(c, iq, iq_stride)) return r;
    if (c->tn_nsrc > 0) return fail(SDR_E_INVALID, "frontend_pre_parts: the context is tuned (the fill by parts is untuned-only)");
    if (!c->rds_on || c->ntaps != FRB_T || (c->flags & SDR_FLAG_FAST_FRONTEND))
        return fail(SDR_E_INVALID, "frontend_pre_parts: needs rds_on, 101 taps and the exact front end");
    if (const int r = plls_parts_check(c, "frontend_pre_parts")) return r;
    hipStream_t s = S(stream);
    const int n = c->info.block_if, ntiles = cdiv(n, FRB_TILE), fe_tiles = frontend_tiles(n);
    nparts = std::min(nparts, ntiles);
    const int p = c->parity ^ 1;
    const FrontendArgs a = frontend_args(c, iq, iq_stride, p);
    if (const int rw = release_wait(c, p, REL_ALL, s)) return rw;
    const int parity0 = c->parity;
    const long long block0 = c->block;
    c->parity = p;                 // the block's buffers (the pre-PLL FIRs read c->parity)
    c->block++;
    // a launch that fails part-way leaves the context on the previous block (nothing was signalled)
    auto undo = [&](int r) { c->parity = parity0; c->block = block0; return r; };
    // part q: the FIR tiles [x0, x1) and the front-end tiles their windows need (tile j writes
    // outputs [adv j, adv j + adv), adv = 64 R - 1); after each part but the last, the count of
    // published tiles. The front end runs in two launches (SDR_FILL_FE_PARTS 0): the first part's
    // tiles, then all the rest with the second part -- one launch fills the chip where three part
    // launches did not, so the block's front end ends ~0.1 ms earlier and the next block's (which
    // continues its I/Q tail) can start (profiles/r06/fill_fe/ab.txt); SDR_FILL_FE_PARTS 1: one
    // front-end launch per part (round 4)
    const int fe_adv = 64 * frontend_tab_r() - 1;
    int fe_done = 0;
    for (int q = 0; q < nparts; q++) {
        const int x0 = q * ntiles / nparts, x1 = (q + 1) * ntiles / nparts;
        const bool fe_split = q < nparts - 1 && (SDR_FILL_FE_PARTS || q == 0);
        const int fe_end = fe_split ? std::min(fe_tiles, cdiv(std::min(x1 * FRB_TILE, n), fe_adv)) : fe_tiles;
        int r = SDR_OK;
        if (fe_end > fe_done) r = frontend_launch(a, s, fe_done, fe_end - fe_done);
        fe_done = std::max(fe_done, fe_end);
        if (!r) r = pre_launch(c, s, x0, x1 - x0);
        if (!r && q < nparts - 1) r = plls_parts_publish(c, x1, s);
        if (r) return undo(r);
    }
    c->st_pre_done = c->rds_pre_done = c->block;
    if (a.env) c->env_block = c->block;   // (every front-end tile ran: the row is whole)
    return sdr_plls_signal(c, stream);   // the whole block: the launch's flag
}

// SDR_FLAG_RDS_QUAD: the quadrature carrier and mixer of the current block (nothing without the flag). Both
// paths of sdr_rds_post launch it before they record REL_RDS: it reads rband and t_rds of this parity.
static int rds_mix_q_launch(sdr_ctx* c, hipStream_t s) {
    if (!(c->flags & SDR_FLAG_RDS_QUAD)) return SDR_OK;
    const int n = c->info.block_if, p = c->parity;
    RdsMixQ a{};
    a.rband = c->rband + p * c->fm_par;
    a.t = c->plain(c->t_rds);
    a.fm_stride = c->fm_stride;
    a.plain_stride = c->plain_stride;
    a.last = c->ipll_q_last + (size_t)p * c->nch;
    a.last_prev = c->ipll_q_last + (size_t)(p ^ 1) * c->nch;
    a.ncoScale = 0.5f;
    a.phaseAdjust = -(float)(M_PI / 2);
    a.rdc = c->rdc_q + p * c->fm_par;
    a.rdc_prev = c->rdc_q + (p ^ 1) * c->fm_par;
    a.rfilt = c->rfilt_q + p * c->rf_par;
    a.rfilt_prev = c->rfilt_q + (p ^ 1) * c->rf_par;
    a.rf_stride = c->rf_stride;
    a.n = n;
    a.n_rds = c->info.n_rds;
    hipLaunchKernelGGL(k_rds_mix_q, dim3(cdiv(n + 1, BLK * MIX_R), c->nch), dim3(BLK), 0, s, a);
    LAUNCH_CHECK();
    return SDR_OK;
}

int sdr_rds_post(sdr_ctx* c, float* rds_clean, size_t rds_stride, void* stream) {
    if (!c) return fail(SDR_E_INVALID, "null context");
    if (const int rf_ = check_failed(c, "rds_post")) return rf_;
    if (c->rds_pll_done != c->block || c->rds_dsp_done == c->block)
        return fail(SDR_E_INVALID, "rds_post: run sdr_rds_pll on a new block first");
    if (const int rf = check_pers_failed(c, "rds_post")) return rf;
    const sdr_info& in = c->info;
    hipStream_t s = S(stream);
    const int n = in.block_if, T = c->ntaps, p = c->parity;
    float* rband = c->rband + p * c->fm_par;
    float* rdc = c->rdc + p * c->fm_par;
    float* rfilt = c->rfilt + p * c->rf_par;
    if (!(c->flags & SDR_FLAG_KEEP_INTERMEDIATES)) {
        // NCO (rds.cpp:119, pll.cpp:52) + delay (:122) + mixer (:125-127) in one pass (k_rds_mix)
        RdsMix a{};
        a.rband = rband;
        a.t = c->plain(c->t_rds);
        a.fm_stride = c->fm_stride;
        a.plain_stride = c->plain_stride;
        a.car = c->pllbuf(c->ipll);
        a.car_prev = c->ipll + (p ^ 1) * c->pll_par;
        a.car_stride = c->pll_stride;
        a.st = c->rds_pll;
        a.ncoScale = 0.5f;                          // rds.cpp:119: fmpll(..., 0.5, 0, 0.001)
        a.phaseAdjust = 0.0f;
        a.rdc = rdc;
        a.rdc_prev = c->rdc + (p ^ 1) * c->fm_par;
        a.rfilt = rfilt;                            // the resampler's history (below)
        a.rfilt_prev = c->rfilt + (p ^ 1) * c->rf_par;
        a.rf_stride = c->rf_stride;
        a.n = n;
        a.n_rds = in.n_rds;
        hipLaunchKernelGGL(k_rds_mix, dim3(cdiv(n + 1, BLK * MIX_R), c->nch), dim3(BLK), 0, s, a);
        LAUNCH_CHECK();
        if (const int rq = rds_mix_q_launch(c, s)) return rq;          // (before the release: it reads rband, t_rds)
        if (const int rr = release_record(c, REL_RDS, s)) return rr;   // rband, t_rds, ipll read
    } else {
        {
            PllJobs jobs{};
            jobs.j[0] = rds_job(c);                   // NCO output of this block's PLL (rds.cpp:119)
            const int r = launch_nco(jobs, 1, n, c->nch, s);
            if (r) return r;
        }
        // delay (rds.cpp:122) + mixer (:125-127) into the extended rds_dc stream
        hipLaunchKernelGGL(k_mix<true>, dim3(cdiv(n, BLK), c->nch), dim3(BLK), 0, s, rband, c->fm_stride,
                           c->pllbuf(c->ipll), c->pll_stride, n, rdc, c->rdc + (p ^ 1) * c->fm_par, c->fm_stride, 50);
        LAUNCH_CHECK();
        if (const int rq = rds_mix_q_launch(c, s)) return rq;
        if (const int rr = release_record(c, REL_RDS, s)) return rr;
        hipLaunchKernelGGL(k_hist_copy, dim3(c->nch), dim3(HIST), 0, s, rfilt, c->rfilt + (p ^ 1) * c->rf_par,
                           c->rf_stride, in.n_rds);
        LAUNCH_CHECK();
    }
    // 247/640 resampler (:130) into the extended rds_filt stream (history: k_rds_mix / k_hist_copy above)
    if (resample_lc_span(c->rdsbb_L, 247, 640) > 64 * RLC_XL || ((c->rdsbb_L + 3) & ~3) > 64 * RLC_HL)
        return fail(SDR_E_INVALID, "rds_post: resampler tile does not fit (L = %d)", c->rdsbb_L);
    dim3 gr(cdiv(in.n_rds, RLC_TN), cdiv(c->nch, 64));
    auto kr = c->rdsbb_all101 ? k_resample_lc<101> : k_resample_lc<0>;
    hipLaunchKernelGGL(kr, gr, dim3(RLC_BLK), resample_lc_lds_bytes(c->rdsbb_L, 247, 640, !c->rdsbb_all101), s, rdc,
                       c->fm_stride, -HIST, c->rdsbb_pp, c->rdsbb_cnt, c->rdsbb_L, c->rds_ptq, in.n_rds, c->nch,
                       rfilt, c->rf_stride);
    LAUNCH_CHECK();
    // RRC (:133) into the context's rds_clean (sdr_rds_bits reads it) and the caller's buffer
    if (T != FRB_T) return fail(SDR_E_INVALID, "rds_post: %d taps", T);
    {
        FirRb f{};
        f.h[0] = c->rrc_h;
        f.y[0] = c->rds_clean;
        f.y_stride[0] = c->clean_stride;
        f.ydup = rds_clean;
        f.ydup_stride = rds_stride;
        f.err = block_poison(c);                    // NaN rows after a persistent PLL or release timeout
        const int r = fir_rb<1, false>(c, rfilt, c->rf_stride, in.n_rds, f, s);
        if (r) return r;
    }
    if (c->flags & SDR_FLAG_RDS_QUAD) {                 // the same resampler and RRC over the quadrature mixer's stream
        float* rfilt_q = c->rfilt_q + p * c->rf_par;
        hipLaunchKernelGGL(kr, gr, dim3(RLC_BLK), resample_lc_lds_bytes(c->rdsbb_L, 247, 640, !c->rdsbb_all101), s,
                           c->rdc_q + p * c->fm_par, c->fm_stride, -HIST, c->rdsbb_pp, c->rdsbb_cnt, c->rdsbb_L, c->rds_ptq,
                           in.n_rds, c->nch, rfilt_q, c->rf_stride);
        LAUNCH_CHECK();
        FirRb f{};
        f.h[0] = c->rrc_h;
        f.y[0] = c->rds_clean_q;
        f.y_stride[0] = c->clean_stride;
        f.err = block_poison(c);
        const int r = fir_rb<1, false>(c, rfilt_q, c->rf_stride, in.n_rds, f, s);
        if (r) return r;
    }
    c->rds_dsp_done = c->block;
    return pers_reader_mark(c, s);
}

int sdr_rds_dsp(sdr_ctx* c, float* rds_clean, size_t rds_stride, void* stream) {
    if (!c) return fail(SDR_E_INVALID, "null context");
    if (c->block < 0 || c->rds_dsp_done == c->block) return fail(SDR_E_INVALID, "rds: no new block");
    int r = sdr_rds_pre(c, stream);
    if (!r) r = sdr_rds_pll(c, stream);
    if (!r) r = sdr_rds_post(c, rds_clean, rds_stride, stream);
    return r;
}

int sdr_rds_bits(sdr_ctx* c, int32_t* offset, int32_t* nsym, uint8_t* symbols, size_t sym_stride, int32_t* nbits,
                 uint8_t* bits, size_t bits_stride, void* stream) {
    if (!c) return fail(SDR_E_INVALID, "null context");
    if (const int rf_ = check_failed(c, "rds_bits")) return rf_;
    if (c->rds_dsp_done != c->block || c->rds_bits_done == c->block)
        return fail(SDR_E_INVALID, "rds_bits: run sdr_rds_dsp on a new block first");
    if (const int rf = check_pers_failed(c, "rds_bits")) return rf;
    const sdr_info& in = c->info;
    hipLaunchKernelGGL(k_rds_bits, dim3(c->nch), dim3(64), (size_t)in.n_rds * sizeof(float),
                       S(stream), c->rds_clean,
                       c->clean_stride, in.n_rds, in.symbol_Fs, c->rds_on, c->dec, offset, nsym, symbols,
                       sym_stride, nbits, bits, bits_stride, block_poison(c),
                       (reinterpret_cast<uintptr_t>(c->rds_clean) % 16 == 0 && c->clean_stride % 4 == 0) ? 1 : 0);
    LAUNCH_CHECK();
    c->rds_bits_done = c->block;
    return pers_reader_mark(c, S(stream));
}

int sdr_push_fm_demod(sdr_ctx* c, const float* fm, size_t fm_stride, void* stream) {
    if (!c || !fm) return fail(SDR_E_INVALID, "null argument");
    if (const int rf_ = check_failed(c, "push_fm_demod")) return rf_;
    const sdr_info& in = c->info;
    const int p = c->parity ^ 1;
    float* dst = c->fm + p * c->fm_par;
    if (const int rw = release_wait(c, p, REL_MONO | REL_STEREO | REL_METER_A, S(stream))) return rw;
    if (const int r = copy_rows(dst, c->fm_stride, fm, fm_stride, in.block_if, c->nch, c->fm + (p ^ 1) * c->fm_par,
                                S(stream)))
        return r;
    c->parity = p;
    c->block++;
    return SDR_OK;
}

}  // extern "C"

