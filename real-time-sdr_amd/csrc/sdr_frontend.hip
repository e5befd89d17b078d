// sdr_frontend.hip -- RF front end of the FM/RDS hot path on MI355X (gfx950):
//   u8 I/Q -> 101-tap FIR /D on I and Q -> FM discriminator       rffrontend.cpp:58-71,
//   filter.cpp:106-121 (convolveFIR), demod.cpp:3-24 (fmDemodNoArctan)
// Exact mode (k_frontend2): the reference's f32 products and sums in tap order, f64 discriminator
// division. Fast mode (k_frontend_mfma): the FIR as an int8 Toeplitz GEMM on the matrix cores.
#include "sdr_internal.h"
#include "demod_phase.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdlib>

#pragma clang fp contract(off)

// Diagnosis builds only (timing, wrong outputs; tools/build_variant.sh FEFLAGS=-DSDR_FE_DIAG=n):
// bit 0 -- k_frontend2 multiplies the raw window words instead of converted samples (no
// conversion), bit 1 -- no discriminator division, bit 2 -- every workgroup stages the same
// L2-resident window. The product build is SDR_FE_DIAG = 0.
#ifndef SDR_FE_DIAG
#define SDR_FE_DIAG 0
#endif

namespace sdrk {
namespace {
// ------------------------------------------------------------------------------------------
// Front end: u8 I/Q -> decimating FIR on I and Q -> discriminator (rffrontend.cpp:58-71,
// filter.cpp:106-121, demod.cpp:3-24). Grid (tiles, nch). A tile computes decimated outputs
// [c0, n1) (c0 = n0-1 so the discriminator has its previous sample) from an LDS window of
// converted I/Q pairs, then writes fm_demod[n0, n1).
// State: tail = last (ntaps-1) I/Q pairs of the previous block (u8, 128 == 0.0f),
//        prev = last decimated (I, Q) of the previous block. Both double-buffered by parity.
// ------------------------------------------------------------------------------------------
// PH: the phase discriminator (SDR_FLAG_PHASE_DEMOD, demod_phase.h) instead of demod.cpp:8-19.
// ENV: the IF envelope row too (SDR_FLAG_IF_ENVELOPE): env[n] = fl(fl(I I) + fl(Q Q)) of every output n
// the tile writes (env: this parity's rows, channel stride fm_stride).
template <bool PH, bool ENV>
__global__ __launch_bounds__(BLK) void k_frontend(
    const uint8_t* __restrict__ iq, size_t iq_stride, const uint8_t* __restrict__ tail_in,
    uint8_t* __restrict__ tail_out, const float2* __restrict__ prev_in, float2* __restrict__ prev_out,
    const float* __restrict__ h, int ntaps, int D, int block_iq, int block_if, int tile,
    float* __restrict__ fm, const float* __restrict__ fm_other, size_t fm_stride, float* __restrict__ env) {
    extern __shared__ float4 smem4[];
    const int ntaps_pad = (ntaps + 3) & ~3;
    float* sh = reinterpret_cast<float*>(smem4);
    const int ch = blockIdx.y;
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * tile;
    const int n1 = min(n0 + tile, block_if);
    const int c0 = max(n0 - 1, 0);
    const int m0 = c0 * D - (ntaps - 1);
    const int m1 = (n1 - 1) * D;
    const int W = m1 - m0 + 1;
    float2* sx = reinterpret_cast<float2*>(sh + ntaps_pad);
    float2* sds = sx + ((W + 1) & ~1);
    const int hist_pairs = ntaps - 1;
    const uint16_t* src = reinterpret_cast<const uint16_t*>(iq + (size_t)ch * iq_stride);
    const uint16_t* tin = reinterpret_cast<const uint16_t*>(tail_in + (size_t)ch * 2 * hist_pairs);

    for (int i = tid; i < ntaps; i += BLK) sh[i] = h[i];
    for (int i = tid; i < W; i += BLK) {
        const int m = m0 + i;
        const uint32_t pr = (m < 0) ? tin[hist_pairs + m] : src[m];
        // float(((u - 128.0) / 128.0)) is exactly (u - 128) * 2^-7
        sx[i] = make_float2(((float)(pr & 0xFFu) - 128.0f) * 0.0078125f, ((float)(pr >> 8) - 128.0f) * 0.0078125f);
    }
    __syncthreads();
    for (int c = c0 + tid; c < n1; c += BLK) {
        const int base = c * D - m0;
        float aI = 0.0f, aQ = 0.0f;
        for (int k = 0; k < ntaps; k++) {
            const float hk = sh[k];
            const float2 v = sx[base - k];
            aI = aI + hk * v.x;
            aQ = aQ + hk * v.y;
        }
        sds[c - c0] = make_float2(aI, aQ);
    }
    __syncthreads();
    float* out = fm + (size_t)ch * fm_stride;
    for (int n = n0 + tid; n < n1; n += BLK) {
        const float2 cur = sds[n - c0];
        const float2 pv = (n == 0) ? prev_in[ch] : sds[n - 1 - c0];
        float r;
        if constexpr (PH) {
            float re, im;
            demod_products(f32x2{cur.x, cur.y}, f32x2{pv.x, pv.y}, re, im);
            r = demod_phase2(f32x2{re, re}, f32x2{im, im}).x;
        } else if ((cur.x == 0) & (cur.y == 0)) {
            r = 0.0f;
        } else {
            const float num = cur.x * (cur.y - pv.y) - cur.y * (cur.x - pv.x);
            const double den = (double)cur.x * (double)cur.x + (double)cur.y * (double)cur.y;
            r = (float)((double)num / den);
        }
        out[n] = r;
        if constexpr (ENV) env[(size_t)ch * fm_stride + n] = cur.x * cur.x + cur.y * cur.y;
    }
    if (n1 == block_if && tid == 0) prev_out[ch] = sds[n1 - 1 - c0];
    if (blockIdx.x == 0) {
        const uint16_t* last = src + (block_iq - hist_pairs);
        uint16_t* tout = reinterpret_cast<uint16_t*>(tail_out + (size_t)ch * 2 * hist_pairs);
        for (int i = tid; i < hist_pairs; i += BLK) tout[i] = last[i];
        const float* o = fm_other + (size_t)ch * fm_stride;
        for (int i = tid; i < HIST; i += BLK) out[i - HIST] = o[block_if - HIST + i];
    }
}

// ------------------------------------------------------------------------------------------
// Front end v2 (register-blocked). Each thread computes R consecutive decimated outputs (I and Q
// as one packed f32 pair) by streaming its input window in DESCENDING sample order: every output
// then still accumulates its taps in ascending k (filter.cpp:110-116), while each input sample is
// converted once and feeds up to R outputs. Conversion: u8 -> signed byte (u ^ 0x80 = u - 128)
// -> f32 m via SDWA sext; with taps pre-scaled by 2^-7 (hs = h/128, exact) the product
// fl(hs*m) equals the reference's fl(h*x), x = (u-128)/128, bit for bit.
//   v_pk_mul_f32 + v_pk_add_f32 (separate roundings, like filter.cpp:115); fast mode is not a
//   variant of this kernel but k_frontend_mfma below, with its own error bound
// A tile computes TILE = 256*R outputs starting one before the first fm_demod sample it writes
// (the discriminator's carry, demod.cpp:16), so tiles advance by TILE-1. The u8 window is staged
// in LDS with coalesced dword loads (D even) or u16 loads (D odd).
// ------------------------------------------------------------------------------------------

// One input sample S (descending) of the register-blocked FIR: up to R independent packed MACs,
// then recursion to S-1 -- complete unrolling with compile-time chunk and tap indices. A
// sched_barrier closes every sample so the scheduler keeps the sample-major order (ILP across the
// R accumulators, each product next to its add) instead of hoisting products or serialising one
// output's chain; the LDS chunk two chunks ahead is read at each chunk boundary.
constexpr int FE_PF = 5;           // tap rows prefetched this many samples ahead (rotating SGPR ring;
                                   // 2-8 and hand-issued batches measured, profiles/r02/fe_exact_ab.txt)
// exact front end: outputs per lane (16 halves the occupancy: 1.54x slower, profiles/r04/ab_fe_r16.txt;
// 12 or 16 with the next tile's window prefetched in registers: slower too, profiles/r04/ab_fe_v4.txt)
#ifndef SDR_FE_R
#define SDR_FE_R 8
#endif
constexpr int FE_R = SDR_FE_R;
// exact discriminator: 1 = reciprocal + Newton step with a tie proof (IEEE division as the fallback),
// 0 = the IEEE f64 division on every output
#ifndef SDR_FE_DISC
#define SDR_FE_DISC 1
#endif
constexpr uint32_t FE_TIE_ULPS = 2048;   // > the fast quotient's 550-ulp error bound, with margin
// {h, h} * m with h one half (HI) of an SGPR pair: v_pk_mul_f32 with a scalar operand whose half
// is broadcast to both lanes by op_sel / op_sel_hi (no VGPR copy of the tap)
__device__ __forceinline__ f32x2 fe_mul_v(double hpair, int hi, f32x2 m) {
    f32x2 r;
    if (hi) asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(r) : "s"(hpair), "v"(m));
    else asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "s"(hpair), "v"(m));
    return r;
}
// (I, Q) of one sample, sign-extended from the bytes of a dword that holds two samples
// (u8 ^ 0x80 == u8 - 128 as int8), converted in program order (volatile asm; the plain C++ form
// saves hazard waits but is no faster, profiles/r02/ab_fe_exact_asm.txt, profiles/r04/ab_fe_v4.txt)
template <int HALF>
__device__ __forceinline__ f32x2 fe_cvt_v(uint32_t w) {
    f32x2 r;
    if (HALF) {
        asm volatile("v_cvt_f32_i32_sdwa %0, sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2\n\t"
                     "v_cvt_f32_i32_sdwa %1, sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3"
                     : "=&v"(r.x), "=v"(r.y) : "v"(w));
    } else {
        asm volatile("v_cvt_f32_i32_sdwa %0, sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0\n\t"
                     "v_cvt_f32_i32_sdwa %1, sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1"
                     : "=&v"(r.x), "=v"(r.y) : "v"(w));
    }
    return r;
}
__device__ __forceinline__ f32x2 fe_add_v(f32x2 a, f32x2 b) {
    f32x2 r;
    asm volatile("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// ------------------------------------------------------------------------------------------
// Fast-mode front end on the matrix cores (SDR_FLAG_FAST_FRONTEND): the decimating FIR as an
// integer GEMM. A wave owns a tile of NB (16, 24 or 32; default 32) blocks of 16 consecutive decimated outputs of one
// channel. Block b's outputs need a 256-sample window w_b (x[D*c_b - 100 + s], s < 256, of which
// 15*D + 101 are used) and y[c_b + i] = sum_s W[i][s] * w_b[s] with the Toeplitz tap matrix
// W[i][s] = h[D*i + 100 - s]. Samples are exact int8 (u8 - 128); the taps are fixed point with
// 2^-F = 2^-(30 - ceil(log2 max|h|)) resolution split into FT_ND = 4 balanced base-256 digits, so
// v_mfma_i32_16x16x64_i8 (rows = 16 outputs, columns = 16 blocks, I and Q as two groups, K = 4 x 64)
// accumulates each digit plane P_0..P_3 exactly in int32 (|P| <= 128 * 128 * 101 < 2^21). The planes
// pair up exactly in int32, hI = (P_0 << 8) + P_1 and lI = (P_2 << 8) + P_3 (|.| < 2^30), and then
// y = fmaf((float)hI, ys * 65536, (float)lI * ys) in f32, ys = 2^-(F+7): two int -> f32 conversions
// and one fma. Both conversions can round: |lI| passes 2^24 on ordinary input, |hI| at full scale
// where F = 33 (2.4e7 at 2.4 MS/s; 1.4e7 < 2^24 where F = 32). y is not the correctly rounded
// convolution. Against the f64 convolution c with the f32 taps, per component, with u = 2^-24 and
// X1 = sum of |x| = |u8 - 128| / 128 over the 101 samples the taps meet:
//   |y - c| <= e = 2^-(F+1) X1                              the taps' fixed-point rounding
//                + 3u (1 + 2^-22) (|c| + 2^-(F+1) X1        the conversions, the products, the fma
//                                  + 514 * 2^(7-F) X1)
// (F = 33 at 2.4 MS/s: 5.8e-11 X1 + 1.8e-7 |c|, at most 5.9e-9 + 1.8e-7 |c|). fm_demod then lies
// within the per-sample bound tol() of tests/fast_fe_model.py of the f64 definition (its docstring
// derives it from the lines of ft_tile_iq): tests/test_gpu_fast_frontend.py on every synth kind,
// full-scale and silent rows, every decimation, both stagings; tests/test_fast_fe_model.py shows
// that a dropped digit plane, a wrong tap digit, a wrong carry row or a wrong prev_in exceeds it.
// North star 1e-5 normwise per block against the f32 reference, RDS bits bit-exact:
// tests/test_gpu_pipeline.py. (3 digits measured 1e-4 on a filter start-up transient.)
// Staging: u8 I/Q pairs -> planar int8 I and Q rows in LDS (v_perm deinterleave); each B
// fragment is then one ds_read_b128 (16 consecutive samples of one component).
// ------------------------------------------------------------------------------------------
// NB = 16-output blocks per wave tile (NB/8 C tiles of 8 blocks). Tile j computes outputs
// c0 .. c0 + 16*NB - 1 with c0 = j*ADV - CARRY and writes the ADV outputs from c0 + CARRY on (the
// CARRY >= 1 before them feed the discriminator). (ADV, CARRY) per D make the first staged sample
// m0 = c0*D - 100 a multiple of 8 (16-byte I/Q groups) on every tile.
constexpr int ft_adv(int D, int NB) { return D == 3 ? 16 * NB - 8 : 16 * NB - 4; }
constexpr int ft_carry(int D) { return D == 10 ? 2 : D == 4 ? 1 : 4; }
constexpr int ft_win(int D, int NB) { return 16 * D * (NB - 1) + 256; }

// One wave tile of the MFMA front end, I and Q of a block in ONE lane (NB a multiple of 16): a
// C tile is 16 blocks, columns = blocks, and the I and Q planes are two MFMA groups with the same A
// fragments, so lane t holds rows 4g..4g+3 of block 16*ct + (t & 15) for both components. The
// discriminator then needs no DPP exchange or component selects, each lane finishes 4 outputs, and
// one pair of shuffles per C tile brings the previous row (lane t-16, or row 15 of the previous block).
template <int D, int NB>
__device__ __forceinline__ void ft_tile_iq(const int8_t* __restrict__ lds, const v4i (&A)[FT_AFRAGS], double yscale,
                                           int c0, int ch, float2 prev_in_ch, float2* __restrict__ prev_out,
                                           int block_if, float* __restrict__ out) {
    static_assert(NB % 16 == 0, "whole 16-block C tiles");
    constexpr int WIN = ft_win(D, NB), ADV = ft_adv(D, NB), CARRY = ft_carry(D);
    const float ys = (float)yscale;
    const int t = threadIdx.x;
    const int n = t & 15, g = t >> 4;
    const int lo = max(c0 + CARRY, 0), hi = min(c0 + CARRY + ADV, block_if);
    // row 4g - 1 of this block (lane t - 16) or row 15 of the previous block (lane 48 + n - 1)
    const int src_lane = g > 0 ? t - 16 : (n > 0 ? t + 47 : t);
    float carry_i = 0.0f, carry_q = 0.0f;             // row 15 of the previous C tile's last block
#pragma unroll 1
    for (int ct = 0; ct < NB / 16; ct++) {
        const int bb = 16 * ct + n;
        v4i aI[FT_ND], aQ[FT_ND];
#pragma unroll
        for (int p = 0; p < FT_ND; p++) { aI[p] = v4i{0, 0, 0, 0}; aQ[p] = v4i{0, 0, 0, 0}; }
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
            const int off = 16 * D * bb + 64 * kk + 16 * g;
            const v4i BI = *reinterpret_cast<const v4i*>(lds + off);
            const v4i BQ = *reinterpret_cast<const v4i*>(lds + WIN + off);
#pragma unroll
            for (int p = 0; p < FT_ND; p++) {
                aI[p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[FT_ND * kk + p], BI, aI[p], 0, 0, 0);
                aQ[p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[FT_ND * kk + p], BQ, aQ[p], 0, 0, 0);
            }
        }
        static_assert(FT_ND == 4, "pairwise recombination assumes 4 digit planes");
        float yI[4], yQ[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            // digits pair up exactly in int32, then one fma in f32 (as ft_tile)
            const int hI = (aI[0][r] << 8) + aI[1][r], lI = (aI[2][r] << 8) + aI[3][r];
            const int hQ = (aQ[0][r] << 8) + aQ[1][r], lQ = (aQ[2][r] << 8) + aQ[3][r];
            yI[r] = __builtin_fmaf((float)hI, ys * 65536.0f, (float)lI * ys);
            yQ[r] = __builtin_fmaf((float)hQ, ys * 65536.0f, (float)lQ * ys);
        }
        const float sI = __shfl(yI[3], src_lane), sQ = __shfl(yQ[3], src_lane);
        const bool first = (t == 0);
        const float pI = first ? carry_i : sI, pQ = first ? carry_q : sQ;
        carry_i = __shfl(yI[3], 63);
        carry_q = __shfl(yQ[3], 63);
        const int cb = c0 + 16 * bb + 4 * g;          // output index of this lane's first row
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int c = cb + r;
            float qI = r == 0 ? pI : yI[r > 0 ? r - 1 : 0], qQ = r == 0 ? pQ : yQ[r > 0 ? r - 1 : 0];
            if (c == 0) {
                qI = prev_in_ch.x;
                qQ = prev_in_ch.y;
            }
            const float cI = yI[r], cQ = yQ[r];
            // demod.cpp:8-19 (fast mode: f32 denominator and a v_rcp_f32 quotient, as ft_tile)
            const float num = cI * (cQ - qQ) - cQ * (cI - qI);
            const float den = cI * cI + cQ * cQ;
            const float q = num * __builtin_amdgcn_rcpf(den);
            v[r] = ((cI == 0.0f) & (cQ == 0.0f)) ? 0.0f : q;
            if (c == block_if - 1) prev_out[ch] = make_float2(cI, cQ);
        }
        if (cb >= lo && cb + 3 < hi && ((cb & 1) == 0)) {
            *reinterpret_cast<float2*>(out + cb) = make_float2(v[0], v[1]);
            *reinterpret_cast<float2*>(out + cb + 2) = make_float2(v[2], v[3]);
        } else {
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (cb + r >= lo && cb + r < hi) out[cb + r] = v[r];
        }
    }
}
template <int D, bool X4, int NB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_frontend_mfma(
    const uint8_t* __restrict__ iq, size_t iq_stride, const uint8_t* __restrict__ tail_in,
    uint8_t* __restrict__ tail_out, const float2* __restrict__ prev_in, float2* __restrict__ prev_out,
    const v4i* __restrict__ afrag, double yscale, int block_iq, int block_if,
    float* __restrict__ fm, const float* __restrict__ fm_other, size_t fm_stride, int tiles_ch,
    const uint32_t* __restrict__ pad, unsigned long long* __restrict__ stamps) {
    static_assert(15 * D + 101 <= 256, "one block's window must fit K = 256");
    // sdr_frontend_timing: this workgroup's start and end on the 100 MHz clock (as k_frontend2)
    if (stamps && threadIdx.x == 0) stamps[2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
    static_assert(NB % 8 == 0, "whole C tiles");
    constexpr int HP = 100, WIN = ft_win(D, NB), G = WIN / 8;
    constexpr int ADV = ft_adv(D, NB), CARRY = ft_carry(D);
    static_assert(CARRY >= 1 && CARRY + ADV <= 16 * NB && WIN % 8 == 0, "tile geometry");
    static_assert(((ADV * D) % 8) == 0 && (((-CARRY * D - HP) % 8) + 8) % 8 == 0, "m0 = 0 mod 8");
    __shared__ __attribute__((aligned(16))) int8_t plane[2][WIN];
    const int t = threadIdx.x;
    const int ch = blockIdx.x / tiles_ch;
    const int j = blockIdx.x - ch * tiles_ch;
    const uint8_t* src = iq + (size_t)ch * iq_stride;
    float* out = fm + (size_t)ch * fm_stride;
    const int c0 = j * ADV - CARRY;
    // ---- stage: groups of 8 I/Q pairs (16 bytes) -> 8 I bytes + 8 Q bytes, signed. All of a
    // lane's window loads are issued first (fully unrolled), then the taps' A fragments (constant,
    // L2-resident, lane-major: every load is 1 KiB contiguous).
    constexpr int GPL = (G + 63) / 64;                // groups per lane
    v4i A[FT_AFRAGS];
    {
        uint4 st[GPL];
        const int m0 = c0 * D - HP;                   // = 0 mod 8
        const uint2* g2 = reinterpret_cast<const uint2*>(src);
        const uint2* t2 = reinterpret_cast<const uint2*>(tail_in + (size_t)ch * 2 * HP);
        const uint2* p2 = reinterpret_cast<const uint2*>(pad);
        const bool interior = (m0 >= 0) && (m0 + WIN <= block_iq);
        if (interior && X4) {                         // 16-byte aligned rows: one dwordx4 per group
            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
            const u32x4* gw = reinterpret_cast<const u32x4*>(src + 2 * m0);
#pragma unroll
            for (int k = 0; k < GPL; k++) {
                const int i = t + 64 * k;
                const u32x4 v = (k < GPL - 1 || i < G) ? __builtin_nontemporal_load(gw + i) : u32x4{0u, 0u, 0u, 0u};
                st[k] = uint4{v.x, v.y, v.z, v.w};
            }
        } else {                                      // 8-byte loads, each from the block, the tail or padding
#pragma unroll
            for (int k = 0; k < GPL; k++) {
                uint2 h[2];
#pragma unroll
                for (int hh = 0; hh < 2; hh++) {
                    const int mm = m0 + 8 * (t + 64 * k) + 4 * hh;
                    const uint2* pa = mm >= 0 ? (mm < block_iq ? g2 + (mm >> 2) : p2)
                                              : (mm >= -HP ? t2 + ((HP + mm) >> 2) : p2);
                    h[hh] = *pa;
                }
                st[k] = uint4{h[0].x, h[0].y, h[1].x, h[1].y};
            }
        }
        // taps after the window: in flight together, the window (older) is waited for first
#pragma unroll
        for (int f = 0; f < FT_AFRAGS; f++) A[f] = afrag[f * 64 + t];
        uint2* pi = reinterpret_cast<uint2*>(plane[0]);
        uint2* pq = reinterpret_cast<uint2*>(plane[1]);
#pragma unroll
        for (int k = 0; k < GPL; k++) {
            const int i = t + 64 * k;
            if (k < GPL - 1 || i < G) {
                const uint4 v = st[k];
                pi[i] = uint2{__builtin_amdgcn_perm(v.y, v.x, 0x06040200u) ^ 0x80808080u,
                              __builtin_amdgcn_perm(v.w, v.z, 0x06040200u) ^ 0x80808080u};
                pq[i] = uint2{__builtin_amdgcn_perm(v.y, v.x, 0x07050301u) ^ 0x80808080u,
                              __builtin_amdgcn_perm(v.w, v.z, 0x07050301u) ^ 0x80808080u};
            }
        }
    }
    __syncthreads();
    ft_tile_iq<D, NB>(plane[0], A, yscale, c0, ch, prev_in[ch], prev_out, block_if, out);
    if (j == 0) {
        const uint16_t* last = reinterpret_cast<const uint16_t*>(src) + (block_iq - HP);
        uint16_t* tout = reinterpret_cast<uint16_t*>(tail_out + (size_t)ch * 2 * HP);
        for (int i = t; i < HP; i += 64) tout[i] = last[i];
        const float* o = fm_other + (size_t)ch * fm_stride;
        for (int i = t; i < HIST; i += 64) out[i - HIST] = o[block_if - HIST + i];
    }
    if (stamps) {   // the end: after this wave's stores have completed
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0) stamps[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
    }
}

// The FIR sweep of one tile: lane t's R outputs from its TWIN-sample window of sign-flipped bytes at
// sw + 2 t R D; 16-byte chunks are read from LDS two ahead of their use.
template <int R, int D>
__device__ __forceinline__ void fe_fir(const uint8_t* __restrict__ sw, const float* __restrict__ hs, f32x2 (&acc)[R]) {
    constexpr int NT = 101, HP = NT - 1;
    constexpr int TWIN = (R - 1) * D + NT;            // samples one thread reads
    constexpr int TCH = (2 * TWIN + 15) / 16;         // 16-byte LDS chunks per thread window
    const int t = threadIdx.x;
    uint4 chunk[TCH];
    const uint4* tw = reinterpret_cast<const uint4*>(sw + 2 * t * R * D);
    chunk[TCH - 1] = tw[TCH - 1];
    if (TCH >= 2) chunk[TCH - 2] = tw[TCH - 2];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = f32x2{0.0f, 0.0f};
    // Taps live in SGPRs: row S of the table holds the R taps sample S meets (uniform across the
    // wave), fetched with scalar loads FE_PF samples ahead into a rotating ring and fed to the packed
    // multiplies as scalar operands (op_sel picks the half of the SGPR pair), so the VALU gets its
    // taps without LDS or VGPR traffic. The tap pointer is made opaque (otherwise every tap load is
    // hoisted and the TWIN*R taps overflow the SGPR file), then declared uniform again with
    // readfirstlane so the loads stay scalar.
    int zero = 0;
    asm volatile("" : "+s"(zero));
    zero = __builtin_amdgcn_readfirstlane(zero);
    const double* hsd = reinterpret_cast<const double*>(hs) + zero;
    double ring[FE_PF][R / 2];
#pragma unroll
    for (int jj = 0; jj < FE_PF; jj++) {
        const int S0 = TWIN - 1 - jj;
#pragma unroll
        for (int q = 0; q < R / 2; q++) ring[S0 % FE_PF][q] = hsd[S0 * (R / 2) + q];
    }
    // sample S's (I, Q) as f32 (u8 - 128, exact) from the LDS chunk registers
    auto sample = [&](int S) -> f32x2 {
        const uint4 c4 = chunk[S >> 3];
        const int dw = (S & 7) >> 1;
        const uint32_t w = dw == 0 ? c4.x : dw == 1 ? c4.y : dw == 2 ? c4.z : c4.w;   // signed bytes (staging)
#if SDR_FE_DIAG & 1
        return f32x2{__builtin_bit_cast(float, w & 0x3F3F3F3Fu), __builtin_bit_cast(float, w & 0x3E3E3E3Eu)};
#else
        return (S & 1) ? fe_cvt_v<1>(w) : fe_cvt_v<0>(w);
#endif
    };
    // one sample of look-ahead: sample S-1 is converted while sample S's MACs issue
    f32x2 m_next = sample(TWIN - 1);
#pragma unroll
    for (int S = TWIN - 1; S >= 0; S--) {
        const int slot = S % FE_PF;
        if (((S & 7) == 7 || S == TWIN - 1) && (S >> 3) >= 2) chunk[(S >> 3) - 2] = tw[(S >> 3) - 2];
        const f32x2 m = m_next;
        // all products of the sample first, then the adds, in program order (volatile asm): no add
        // waits on the product issued just before it (filter.cpp:115: multiply, then add)
        f32x2 prod[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int k = r * D + HP - S;
            if (k >= 0 && k < NT) prod[r] = fe_mul_v(ring[slot][r >> 1], r & 1, m);
        }
        if (S > 0) m_next = sample(S - 1);
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int k = r * D + HP - S;
            if (k >= 0 && k < NT) acc[r] = fe_add_v(acc[r], prod[r]);
        }
        if (S - FE_PF >= 0) {
#pragma unroll
            for (int q = 0; q < R / 2; q++) ring[slot][q] = hsd[(S - FE_PF) * (R / 2) + q];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The discriminator (demod.cpp:8-19) of lane t's R outputs c0 + t R + r and their stores into out
// (fm_demod of the channel; c0 is the tile's carry output, never written); the block's last (I, Q)
// goes to prev_out. PH: the phase discriminator (SDR_FLAG_PHASE_DEMOD, demod_phase.h) instead -- all
// f32, two outputs per packed polynomial, none of the f64 reciprocal, tie key or division fallback.
// ENV: the IF envelope row too (SDR_FLAG_IF_ENVELOPE): env[c] = fl(fl(I I) + fl(Q Q)) of every output c
// whose fm sample is stored, by the same rule and with the same aligned float2 fast path (env: the
// channel's row, laid out as out is; unused without ENV).
template <int R, bool PH, bool ENV>
__device__ __forceinline__ void fe_disc_store(const f32x2 (&acc)[R], int c0, int ch, const float2* __restrict__ prev_in,
                                              float2* __restrict__ prev_out, float* __restrict__ out,
                                              float* __restrict__ env, int block_if) {
    // ---- discriminator (demod.cpp:8-19); the previous output of lane t's first comes from t-1
    const f32x2 left = f32x2{__shfl_up(acc[R - 1].x, 1), __shfl_up(acc[R - 1].y, 1)};
    const int t = threadIdx.x;
    const int cbase = c0 + t * R;
    float v[R];
#if SDR_FE_DIAG & 2
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = acc[r].x + ((r > 0) ? acc[r > 0 ? r - 1 : 0] : left).y;
#else
    // the previous sample of output r; output 0 of the block (its previous sample is the last block's
    // carry, prev_in) can only be output 1 of lane 0 of tile 0 (c0 = j*ADV - 1 >= -1)
    auto prev = [&](int r) -> f32x2 {
        f32x2 pv = (r > 0) ? acc[r > 0 ? r - 1 : 0] : left;
        if (r == 1 && cbase == -1) {
            const float2 p = prev_in[ch];
            pv = f32x2{p.x, p.y};
        }
        return pv;
    };
    if constexpr (PH) {
        static_assert(R % 2 == 0, "outputs are finished in pairs");
#pragma unroll
        for (int r = 0; r < R; r += 2) {
            float re0, im0, re1, im1;
            demod_products(acc[r], prev(r), re0, im0);
            demod_products(acc[r + 1], prev(r + 1), re1, im1);
            const f32x2 ph = demod_phase2(f32x2{re0, re1}, f32x2{im0, im1});
            v[r] = ph.x;
            v[r + 1] = ph.y;
        }
    } else {                                         // the reference's discriminator (its lines keep their indentation)
#if SDR_FE_DISC
    // The reference's value is RN32(RN64(num / den)), den = RN64(I^2 + Q^2) (pow(x, 2.0) is exact
    // in f64, so den is one fma). Instead of the IEEE f64 division: q = RN64(num * r1), r1 = 1/den
    // from v_rcp_f64 (~2^-23 relative) refined by one Newton step, so |q / (num/den) - 1| < 2^-43.9,
    // i.e. < 550 ulps of q. RN32(q) equals the reference's value unless q lies within FE_TIE_ULPS
    // ulps of an f32 rounding tie (the tie key) or rounds to an f32 subnormal: a lane with any such
    // output recomputes its outputs by the division (a branch taken by ~1e-5 of the lanes).
    uint32_t kmin = 0xFFFFFFFFu;
    bool sub = false;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const f32x2 cur = acc[r], pv = prev(r);
        const float num = cur.x * (cur.y - pv.y) - cur.y * (cur.x - pv.x);
        const double dI = (double)cur.x, dQ = (double)cur.y;
        const double den = __builtin_fma(dI, dI, dQ * dQ);
        const double r0 = __builtin_amdgcn_rcp(den);
        const double r1 = __builtin_fma(r0, __builtin_fma(-den, r0, 1.0), r0);
        const double q = (double)num * r1;
        const float vq = (float)q;
        const uint32_t key = ((uint32_t)__builtin_bit_cast(uint64_t, q) << 3) + (0x80000000u + 8u * FE_TIE_ULPS);
        kmin = key < kmin ? key : kmin;
        sub |= __builtin_amdgcn_classf(vq, 0x90);   // negative or positive f32 subnormal
        v[r] = den == 0.0 ? 0.0f : vq;              // (I, Q) = (0, 0): demod.cpp:15-16
    }
    if (kmin <= 16u * FE_TIE_ULPS || sub) {
#else
    {
#endif
#pragma unroll
        for (int r = 0; r < R; r++) {
            const f32x2 cur = acc[r], pv = prev(r);
            if ((cur.x == 0) & (cur.y == 0)) {
                v[r] = 0.0f;
            } else {
                const float num = cur.x * (cur.y - pv.y) - cur.y * (cur.x - pv.x);
                const double den = (double)cur.x * (double)cur.x + (double)cur.y * (double)cur.y;
                v[r] = (float)((double)num / den);
            }
        }
    }
    }                                                // if constexpr (PH) .. else
#endif
    float e[ENV ? R : 1];                            // the IF power of each output: a square each, one sum
    (void)e;
    if constexpr (ENV) {
#pragma unroll
        for (int r = 0; r < R; r++) e[r] = acc[r].x * acc[r].x + acc[r].y * acc[r].y;
    }
    if (t > 0 && cbase + R < block_if) {             // all R outputs written, none the block's last
        if ((reinterpret_cast<uintptr_t>(out + cbase) & 7) == 0) {
#pragma unroll
            for (int r = 0; r < R; r += 2) *reinterpret_cast<float2*>(out + cbase + r) = make_float2(v[r], v[r + 1]);
        } else {
#pragma unroll
            for (int r = 0; r < R; r++) out[cbase + r] = v[r];
        }
        if constexpr (ENV) {
            if ((reinterpret_cast<uintptr_t>(env + cbase) & 7) == 0) {
#pragma unroll
                for (int r = 0; r < R; r += 2) *reinterpret_cast<float2*>(env + cbase + r) = make_float2(e[r], e[r + 1]);
            } else {
#pragma unroll
                for (int r = 0; r < R; r++) env[cbase + r] = e[r];
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int c = cbase + r;
            if (c > c0 && c >= 0 && c < block_if) {
                out[c] = v[r];
                if constexpr (ENV) env[c] = e[r];
            }
            if (c == block_if - 1) prev_out[ch] = make_float2(acc[r].x, acc[r].y);
        }
    }
}

// Exact front end, one tile per workgroup (64 lanes): a tile = 64*R decimated outputs starting one
// before the first fm_demod sample it writes (the discriminator's carry, demod.cpp:16); tiles
// advance by 64*R-1. The tile's u8 window goes HBM -> registers (coalesced dwords) -> LDS, then every
// lane sweeps its R outputs' window. Boundary tiles (the first reads the previous block's tail, the
// last runs into the padding, u8 128 = 0.0f) stage per dword from the block, the tail or the pad.
// Tiles j0 .. j0+jn-1 of every channel (blockIdx.x = ch*jn + j - j0): the whole block (j0 = 0, jn =
// tiles per channel) or one part of it (sdr_frontend_pre_parts, the pipeline fill).
template <int R, int D, bool PH, bool ENV>
__global__ __launch_bounds__(64) void k_frontend2(
    const uint8_t* __restrict__ iq, size_t iq_stride, const uint8_t* __restrict__ tail_in,
    uint8_t* __restrict__ tail_out, const float2* __restrict__ prev_in, float2* __restrict__ prev_out,
    const float* __restrict__ hs, int block_iq, int block_if,
    float* __restrict__ fm, const float* __restrict__ fm_other, size_t fm_stride, int j0, int jn,
    const uint32_t* __restrict__ pad, unsigned long long* __restrict__ stamps, float* __restrict__ env) {
    constexpr int NT = 101, HP = NT - 1, NTH = 64;
    // sdr_frontend_timing: this workgroup's start and end on the 100 MHz clock (the launch's span is
    // the earliest start to the latest end, computed on the host)
    if (stamps && threadIdx.x == 0) stamps[2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
    constexpr int TILE = NTH * R;
    constexpr int ADV = TILE - 1;
    constexpr int WIN = (TILE - 1) * D + NT;          // staged samples (u8 I/Q pairs)
    constexpr int NG = (2 * WIN + 3) / 4;             // dwords of one tile window
    constexpr int PER = (NG + NTH - 1) / NTH;         // dwords per lane
    constexpr int LDS_BYTES = ((2 * WIN + 15) / 16) * 16 + 32;
    __shared__ __attribute__((aligned(16))) uint8_t sw[LDS_BYTES];
    const int t = threadIdx.x;
    const int ch = (int)blockIdx.x / jn, j = j0 + (int)blockIdx.x - ch * jn;
    const int c0 = j * ADV - 1;                       // first decimated output (the carry)
    const int m0 = c0 * D - HP;                       // first staged sample
    const uint8_t* src = iq + (size_t)ch * iq_stride;
#if SDR_FE_DIAG & 4
    // diagnosis: every workgroup stages channel 0's second tile (L2-resident input, staging latency
    // without HBM misses)
    const int m0s = ADV * D - D - HP;
    const uint8_t* srcs = iq;
#else
    const int m0s = m0;
    const uint8_t* srcs = src;
#endif
    {
        // window -> LDS (lane t holds dwords t, t+64, ...). Every I/Q sample is one u16; samples
        // before the block come from the previous block's tail, samples past its end are u8 128.
        // With D even the window starts on an even sample, so each dword is wholly in the block, in
        // the tail or in the padding: one load (or constant) per dword.
        uint32_t* sd = reinterpret_cast<uint32_t*>(sw);
        const uint8_t* tin = tail_in + (size_t)ch * 2 * HP;
        if (D % 2 == 0) {
            if (m0s >= 0 && m0s + WIN <= block_iq) {
                const uint32_t* g = reinterpret_cast<const uint32_t*>(srcs + 2 * m0s);
                uint32_t pf[PER];
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    const int i = t + NTH * k;
                    pf[k] = (k < PER - 1 || i < NG) ? __builtin_nontemporal_load(g + i) : 0u;
                }
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    const int i = t + NTH * k;
                    if (k < PER - 1 || i < NG) sd[i] = pf[k] ^ 0x80808080u;
                }
            } else {
                const uint32_t* gs = reinterpret_cast<const uint32_t*>(src);
                const uint32_t* gt = reinterpret_cast<const uint32_t*>(tin);
                for (int i = t; i < NG; i += NTH) {
                    const int mm = m0 + 2 * i;
                    const uint32_t* pa = mm >= 0 ? (mm < block_iq ? gs + (mm >> 1) : pad)
                                                 : (mm >= -HP ? gt + ((HP + mm) >> 1) : pad);
                    sd[i] = *pa ^ 0x80808080u;
                }
            }
        } else {
            const uint16_t* s16 = reinterpret_cast<const uint16_t*>(src);
            const uint16_t* t16 = reinterpret_cast<const uint16_t*>(tin);
            for (int i = t; i < NG; i += NTH) {
                uint32_t v = 0;
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int m = m0 + 2 * i + h;
                    const uint16_t* pa = m >= 0 ? s16 + m : t16 + (HP + m);
                    if (m < -HP || m >= block_iq) pa = reinterpret_cast<const uint16_t*>(pad);
                    v |= (uint32_t)*pa << (16 * h);
                }
                sd[i] = v ^ 0x80808080u;
            }
        }
    }
    __syncthreads();
    f32x2 acc[R];
    fe_fir<R, D>(sw, hs, acc);
    fe_disc_store<R, PH, ENV>(acc, c0, ch, prev_in, prev_out, fm + (size_t)ch * fm_stride,
                              ENV ? env + (size_t)ch * fm_stride : nullptr, block_if);
    float* out = fm + (size_t)ch * fm_stride;
    if (j == 0) {
        const uint16_t* last = reinterpret_cast<const uint16_t*>(src) + (block_iq - HP);
        uint16_t* tout = reinterpret_cast<uint16_t*>(tail_out + (size_t)ch * 2 * HP);
        for (int i = t; i < HP; i += NTH) tout[i] = last[i];
        const float* o = fm_other + (size_t)ch * fm_stride;
        for (int i = t; i < HIST; i += NTH) out[i - HIST] = o[block_if - HIST + i];
    }
    if (stamps) {   // the end: after this wave's stores have completed
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0) stamps[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
    }
}

// ------------------------------------------------------------------------------------------
// Tuned front end (sdr_frontend_tuned): channel ch listens to source row src[ch] and is shifted by
// khz[ch] kHz before the same FIR and discriminator. With N = rf_Fs / 1000 (2400, 1440, 1152 for
// D = 10, 4, 3) sample n of the stream is multiplied by T[(khz n) mod N] = (cos, sin)(2 pi i / N):
//   y_I = fl(fl(x_I c) + fl(x_Q s)),  y_Q = fl(fl(x_Q c) - fl(x_I s))       (no FMA)
// Same tile scheme as k_frontend2 (64 lanes, R outputs per lane, tiles advance by 64 R - 1), but the
// staging phase converts and rotates every sample of the tile's window ONCE and keeps it in LDS as
// an f32 pair; the FIR sweep then reads f32 pairs (no per-lane conversion). Samples are kept as
// u8 - 128 (not / 128) against taps pre-scaled by 2^-7 like k_frontend2's: the power of two
// commutes with every rounding of the mixer and of the products (nothing here is near the
// subnormal range), so the sums are the reference's bit for bit.
// Rotator: the quarter table Q[k] = RN32(cos(2 pi k / N)), 0 <= k <= N/4, in LDS (2.4 KiB for
// N = 2400); cos and sin of any index follow by the quadrant symmetries (sin(k) = Q[N/4 - k]), the
// same rule the host uses for sdr_tuner_table, so both hold the same values. The index advances
// incrementally (an add and an unsigned minimum per step; one constant modulus per lane and tile).
// Measured and dropped: the first half of the table as (cos, sin) pairs in LDS (9.4 KiB, one 8-byte
// read and a sign flip per sample, fewer VALU instructions but 5 instead of 6 waves per CU):
// 0.206 against 0.188 ms for 1024 channels on 128 rows (profiles/r07/tuner/).
// Measured and dropped too: 16 bytes of LDS padding after every R D samples, so that the 16 lanes of
// one pass of a 16-byte window read (lane stride 320 bytes at D = 10, four lanes per bank group)
// cover 64 different banks: 0.191 against 0.188 ms, no gain -- the LDS reads do not bound the kernel.
// Grid: logical workgroup L = pos * tiles + j, pos the channel's place in the order sorted by
// source row, so the stations of one row are neighbours; hardware workgroup b runs L = (b % nxcc) *
// per + b / nxcc because consecutive workgroups are dealt round-robin over the XCCs (sdr_internal.h,
// CuPlacement) and each XCC has its own L2: one XCC then runs consecutive L, fetches a row's window
// from HBM once and serves its other stations from its L2.
// LDS: 8 bytes per staged sample, 80 bytes per output at D = 10. R = 4: 23.6 KiB per workgroup, 6
// waves per CU of the 160 KiB; R = 8 (the untuned kernel's): 44 KiB, 3 waves per CU, fewer than one
// per SIMD. SDR_TN_R selects it for A/B builds.
// ------------------------------------------------------------------------------------------
#ifndef SDR_TN_R
#define SDR_TN_R 4
#endif
constexpr int TN_R = SDR_TN_R;
constexpr int TN_PFC = 4;          // 16-byte LDS chunks (2 samples) read this many ahead of their use
constexpr int tn_n(int D) { return D == 10 ? 2400 : D == 4 ? 1440 : 1152; }

// The FIR sweep over an f32 window: as fe_fir (descending samples, taps in SGPRs), samples read
// from LDS as (I, Q) f32 pairs, two per 16-byte chunk.
template <int R, int D>
__device__ __forceinline__ void tn_fir(const float* __restrict__ sy, const float* __restrict__ hs, f32x2 (&acc)[R]) {
    constexpr int NT = 101, HP = NT - 1;
    constexpr int TWIN = (R - 1) * D + NT;            // samples one thread reads
    constexpr int TCH = (TWIN + 1) / 2;               // 16-byte LDS chunks per thread window
    static_assert((R * D) % 2 == 0 && R % 2 == 0, "lane windows start on 16-byte chunks; taps come in pairs");
    static_assert(TCH > TN_PFC, "prefetch depth");
    const int t = threadIdx.x;
    float4 chunk[TCH];
    const float4* tw = reinterpret_cast<const float4*>(sy + 2 * t * R * D);
#pragma unroll
    for (int q = 1; q <= TN_PFC; q++) chunk[TCH - q] = tw[TCH - q];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = f32x2{0.0f, 0.0f};
    int zero = 0;                                     // (opaque, then uniform again: see fe_fir)
    asm volatile("" : "+s"(zero));
    zero = __builtin_amdgcn_readfirstlane(zero);
    const double* hsd = reinterpret_cast<const double*>(hs) + zero;
    double ring[FE_PF][R / 2];
#pragma unroll
    for (int jj = 0; jj < FE_PF; jj++) {
        const int S0 = TWIN - 1 - jj;
#pragma unroll
        for (int q = 0; q < R / 2; q++) ring[S0 % FE_PF][q] = hsd[S0 * (R / 2) + q];
    }
#pragma unroll
    for (int S = TWIN - 1; S >= 0; S--) {
        const int slot = S % FE_PF;
        if (((S & 1) == 1 || S == TWIN - 1) && (S >> 1) >= TN_PFC) chunk[(S >> 1) - TN_PFC] = tw[(S >> 1) - TN_PFC];
        const float4 c4 = chunk[S >> 1];
        const f32x2 m = (S & 1) ? f32x2{c4.z, c4.w} : f32x2{c4.x, c4.y};
        f32x2 prod[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int k = r * D + HP - S;
            if (k >= 0 && k < NT) prod[r] = fe_mul_v(ring[slot][r >> 1], r & 1, m);
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int k = r * D + HP - S;
            if (k >= 0 && k < NT) acc[r] = fe_add_v(acc[r], prod[r]);
        }
        if (S - FE_PF >= 0) {
#pragma unroll
            for (int q = 0; q < R / 2; q++) ring[slot][q] = hsd[(S - FE_PF) * (R / 2) + q];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// tune[pos] = {channel, source row, khz mod N, 1: this channel stores its row's tail}
template <int R, int D, bool PH, bool ENV>
__global__ __launch_bounds__(64) void k_frontend_tuned(
    const uint8_t* __restrict__ iq, size_t iq_stride, const uint8_t* __restrict__ tail_in,
    uint8_t* __restrict__ tail_out, const float2* __restrict__ prev_in, float2* __restrict__ prev_out,
    const float* __restrict__ hs, const float* __restrict__ qtab, const int4* __restrict__ tune, int phase0,
    int block_iq, int block_if, float* __restrict__ fm, const float* __restrict__ fm_other, size_t fm_stride,
    int tiles, int total, int per, int nxcc, const uint32_t* __restrict__ pad, unsigned long long* __restrict__ stamps,
    float* __restrict__ env) {
    constexpr int NT = 101, HP = NT - 1, NTH = 64;
    constexpr int N = tn_n(D), Q4 = N / 4;
    if (stamps && threadIdx.x == 0) stamps[2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
    constexpr int TILE = NTH * R;
    constexpr int ADV = TILE - 1;
    constexpr int WIN = (TILE - 1) * D + NT;          // staged samples
    constexpr int NP = (WIN + 1) / 2;                 // sample pairs (16-byte LDS chunks)
    constexpr int PER = (NP + NTH - 1) / NTH;         // pairs per lane
    __shared__ __attribute__((aligned(16))) float4 sy4[NP];
    __shared__ float sq[Q4 + 1];
    const int t = threadIdx.x;
    const int b = (int)blockIdx.x;
    const int L = (b % nxcc) * per + b / nxcc;
    if (L >= total) {                                 // the grid is rounded up to whole XCC shares
        if (stamps && t == 0) stamps[2 * b + 1] = __builtin_amdgcn_s_memrealtime();
        return;
    }
    const int pos = L / tiles, j = L - pos * tiles;
    const int4 tn = tune[pos];
    const int ch = tn.x, srow = tn.y, kpos = tn.z;
    const int c0 = j * ADV - 1;                       // first decimated output (the carry)
    const int m0 = c0 * D - HP;                       // first staged sample (>= -D - HP)
    const uint8_t* src = iq + (size_t)srow * iq_stride;
    const uint8_t* tin = tail_in + (size_t)srow * 2 * HP;
    for (int i = t; i <= Q4; i += NTH) sq[i] = qtab[i];
    // ---- the window's u8 pairs -> registers (one dword = two samples per lane and step)
    uint32_t pf[PER];
    const bool interior = m0 >= 0 && m0 + 2 * NP <= block_iq;
    if (interior && (reinterpret_cast<uintptr_t>(src + 2 * m0) & 3) == 0) {
        const uint32_t* g = reinterpret_cast<const uint32_t*>(src + 2 * m0);
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int i = t + NTH * k;
            pf[k] = (k < PER - 1 || i < NP) ? g[i] : 0x80808080u;
        }
    } else {
        // per sample from the block, the row's tail (the 100 samples before the block) or u8 128
        const uint16_t* s16 = reinterpret_cast<const uint16_t*>(src);
        const uint16_t* t16 = reinterpret_cast<const uint16_t*>(tin);
        const uint16_t* p16 = reinterpret_cast<const uint16_t*>(pad);
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int i = t + NTH * k;
            uint32_t v = 0x80808080u;
            if (k < PER - 1 || i < NP) {
                v = 0;
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int m = m0 + 2 * i + h;
                    const uint16_t* pa = (m >= 0 && m < block_iq) ? s16 + m : (m < 0 && m >= -HP) ? t16 + (HP + m) : p16;
                    v |= (uint32_t)*pa << (16 * h);
                }
            }
            pf[k] = v;
        }
    }
    __syncthreads();                                  // the table is in LDS
    // ---- convert, rotate, store. Sample m of the block is sample n = B block_iq + m of the stream;
    // nn = n mod N of this lane's first sample (phase0 = (B block_iq) mod N, m0 + N > 0), idx = (khz n) mod N
    {
        const uint32_t nn = (uint32_t)(phase0 + m0 + 2 * t + N) % (uint32_t)N;
        int idxA = (int)(((uint32_t)kpos * nn) % (uint32_t)N);
        const int step = (int)(((uint32_t)kpos * (2u * NTH)) % (uint32_t)N);
        // (c, s) of index i by the quadrant symmetries (0 - x: a zero stays +0, as in sdr_tuner_table)
        auto rot = [&](uint32_t i, float& c, float& sn) {
            const int q = (i >= 2u * Q4) ? ((i >= 3u * Q4) ? 3 : 2) : ((i >= (uint32_t)Q4) ? 1 : 0);
            const int r = (int)i - q * Q4;
            const float a = sq[r], bq = sq[Q4 - r];   // cos and sin of 2 pi r / N
            c = (q & 1) ? bq : a;
            sn = (q & 1) ? a : bq;
            if (q == 1 || q == 2) c = 0.0f - c;
            if (q >= 2) sn = 0.0f - sn;
        };
        uint32_t ia = (uint32_t)idxA;
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int i = t + NTH * k;
            const uint32_t ib = min(ia + (uint32_t)kpos, ia + (uint32_t)kpos - (uint32_t)N);
            const uint32_t w = pf[k] ^ 0x80808080u;               // u8 - 128 as signed bytes
            const f32x2 x0 = fe_cvt_v<0>(w), x1 = fe_cvt_v<1>(w);
            float c0f, s0f, c1f, s1f;
            rot(ia, c0f, s0f);
            rot(ib, c1f, s1f);
            float4 o;
            o.x = x0.x * c0f + x0.y * s0f;
            o.y = x0.y * c0f - x0.x * s0f;
            o.z = x1.x * c1f + x1.y * s1f;
            o.w = x1.y * c1f - x1.x * s1f;
            if (k < PER - 1 || i < NP) sy4[i] = o;
            ia = min(ia + (uint32_t)step, ia + (uint32_t)step - (uint32_t)N);
        }
    }
    __syncthreads();
    f32x2 acc[R];
    tn_fir<R, D>(reinterpret_cast<const float*>(sy4), hs, acc);
    float* out = fm + (size_t)ch * fm_stride;
    fe_disc_store<R, PH, ENV>(acc, c0, ch, prev_in, prev_out, out, ENV ? env + (size_t)ch * fm_stride : nullptr, block_if);
    if (j == 0) {
        if (tn.w) {                                   // one channel per source row keeps the row's tail
            const uint16_t* last = reinterpret_cast<const uint16_t*>(src) + (block_iq - HP);
            uint16_t* tout = reinterpret_cast<uint16_t*>(tail_out + (size_t)srow * 2 * HP);
            for (int i = t; i < HP; i += NTH) tout[i] = last[i];
        }
        const float* o = fm_other + (size_t)ch * fm_stride;
        for (int i = t; i < HIST; i += NTH) out[i - HIST] = o[block_if - HIST + i];
    }
    if (stamps) {   // the end: after this wave's stores have completed
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0) stamps[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
    }
}

size_t frontend_lds_bytes(int ntaps, int tile, int D) {
    const int ntaps_pad = (ntaps + 3) & ~3;
    const int W = tile * D + ntaps;                  // window incl. the extra output at n0-1
    return (size_t)ntaps_pad * 4 + (size_t)((W + 1) & ~1) * 8 + (size_t)(tile + 1) * 8 + 64;
}

}  // namespace

// One block of every channel (the RF_frontend loop body), or tiles [j0, j0 + jn) of it (a part of
// the pipeline fill, sdr_frontend_pre_parts): picks the kernel for the context's numerics and
// decimation.
int frontend_tiles(int block_if) { return cdiv(block_if + 1, 64 * FE_R - 1); }
int frontend_tab_r() { return FE_R; }

int frontend_launch(const FrontendArgs& a, hipStream_t s, int j0, int jn) {
    const uint8_t* iq = a.iq;
    const size_t iq_stride = a.iq_stride;
    const uint8_t* tail_in = a.tail_in;
    uint8_t* tail_out = a.tail_out;
    const float2* prev_in = a.prev_in;
    float2* prev_out = a.prev_out;
    float* fm_p = a.fm;
    const float* fm_o = a.fm_other;
    const int tiles_ch = frontend_tiles(a.block_if);
    if (jn <= 0) { j0 = 0; jn = tiles_ch; }
    if (j0 < 0 || j0 + jn > tiles_ch) return fail(SDR_E_INVALID, "frontend: tiles [%d, %d) of %d", j0, j0 + jn, tiles_ch);
    const dim3 g2(jn * a.nch);
    // sdr_frontend_timing: k_frontend2 and k_frontend_mfma stamp each workgroup's start and end
    // (a.stamps); the generic kernel records HIP events with the launch (hipExtLaunchKernelGGL: the
    // start event is a marker ahead of the dispatch, so its span exceeds the kernel's by the marker's
    // latency, ~9 us)
    // a.env (SDR_FLAG_IF_ENVELOPE) picks the instantiations that also store the IF envelope row
#define FE2E(DD, PP, EE)                                                                                      \
    hipExtLaunchKernelGGL((k_frontend2<FE_R, DD, PP, EE>), g2, dim3(64), 0, s, a.ev0, a.ev1, 0, iq, iq_stride, tail_in, \
                          tail_out, prev_in, prev_out, a.hs, a.block_iq, a.block_if, fm_p, fm_o, a.fm_stride, j0, jn, \
                          a.pad80, a.stamps, a.env)
#define FE2(DD, PP) do { if (a.env) FE2E(DD, PP, true); else FE2E(DD, PP, false); } while (0)
    if (a.fast) {
        if (j0 != 0 || jn != tiles_ch) return fail(SDR_E_INVALID, "frontend: parts need the exact front end");
        const v4i* af = static_cast<const v4i*>(a.afrag);
        // 16-byte I/Q group loads need 16-byte aligned rows (e.g. a row stride of 147008 for mode 0)
        const bool x4 = (iq_stride % 16 == 0) && (reinterpret_cast<uintptr_t>(iq) % 16 == 0);
        constexpr int NB = FT_NB;
#define FEM(DD, XX)                                                                                          \
        hipExtLaunchKernelGGL((k_frontend_mfma<DD, XX, NB>), dim3(cdiv(a.block_if, ft_adv(DD, NB)) * a.nch),   \
                              dim3(64), 0, s, a.ev0, a.ev1, 0, iq, iq_stride, tail_in, tail_out, prev_in, prev_out, af, \
                              a.yscale, a.block_iq, a.block_if, fm_p, fm_o, a.fm_stride,                            \
                              cdiv(a.block_if, ft_adv(DD, NB)), a.pad80, a.stamps)
        if (a.D == 10) { if (x4) FEM(10, true); else FEM(10, false); }
        else if (a.D == 4) { if (x4) FEM(4, true); else FEM(4, false); }
        else { if (x4) FEM(3, true); else FEM(3, false); }
#undef FEM
    } else if (a.ntaps == 101 && a.D == 10) {
        if (a.phase) FE2(10, true); else FE2(10, false);
    } else if (a.ntaps == 101 && a.D == 4) {
        if (a.phase) FE2(4, true); else FE2(4, false);
    } else if (a.ntaps == 101 && a.D == 3) {
        if (a.phase) FE2(3, true); else FE2(3, false);
    } else {
        if (j0 != 0 || jn != tiles_ch) return fail(SDR_E_INVALID, "frontend: parts need 101 taps");
        const int tile = FIR_TILE;
        dim3 grid(cdiv(a.block_if, tile), a.nch);
        const size_t lds = frontend_lds_bytes(a.ntaps, tile, a.D);
#define FEG(PP, EE)                                                                                           \
        hipExtLaunchKernelGGL((k_frontend<PP, EE>), grid, dim3(BLK), (uint32_t)lds, s, a.ev0, a.ev1, 0, iq, iq_stride, \
                              tail_in, tail_out, prev_in, prev_out, a.h, a.ntaps, a.D, a.block_iq, a.block_if, tile,   \
                              fm_p, fm_o, a.fm_stride, a.env)
        if (a.env) { if (a.phase) FEG(true, true); else FEG(false, true); }
        else { if (a.phase) FEG(true, false); else FEG(false, false); }
#undef FEG
    }
#undef FE2
#undef FE2E
    LAUNCH_CHECK();
    return SDR_OK;
}

// ---- tuned front end
int frontend_tuned_r() { return TN_R; }
int frontend_tuned_n(int D) { return tn_n(D); }
static int tuned_tiles(int block_if) { return cdiv(block_if + 1, 64 * TN_R - 1); }
// hardware workgroups: the logical ones rounded up to whole XCC shares (k_frontend_tuned)
int frontend_tuned_wgs(int block_if, int nch, int nxcc) {
    nxcc = std::max(nxcc, 1);
    return cdiv(tuned_tiles(block_if) * nch, nxcc) * nxcc;
}

int frontend_tuned_launch(const FrontendArgs& a, const float* ht, const float* qtab, const int32_t* tune, int phase0,
                          int nxcc, hipStream_t s) {
    if (a.ntaps != 101 || (a.D != 10 && a.D != 4 && a.D != 3))
        return fail(SDR_E_INVALID, "frontend_tuned: needs 101 taps and a decimation of 10, 4 or 3");
    nxcc = std::max(nxcc, 1);
    const int tiles = tuned_tiles(a.block_if), total = tiles * a.nch, per = cdiv(total, nxcc);
    const dim3 g(per * nxcc);
    const int4* tn = reinterpret_cast<const int4*>(tune);
#define FETE(DD, PP, EE)                                                                                          \
    hipLaunchKernelGGL((k_frontend_tuned<TN_R, DD, PP, EE>), g, dim3(64), 0, s, a.iq, a.iq_stride, a.tail_in, a.tail_out, \
                       a.prev_in, a.prev_out, ht, qtab, tn, phase0, a.block_iq, a.block_if, a.fm, a.fm_other,         \
                       a.fm_stride, tiles, total, per, nxcc, a.pad80, a.stamps, a.env)
#define FET(DD, PP) do { if (a.env) FETE(DD, PP, true); else FETE(DD, PP, false); } while (0)
    if (a.D == 10) { if (a.phase) FET(10, true); else FET(10, false); }
    else if (a.D == 4) { if (a.phase) FET(4, true); else FET(4, false); }
    else { if (a.phase) FET(3, true); else FET(3, false); }
#undef FET
#undef FETE
    LAUNCH_CHECK();
    return SDR_OK;
}

int frontend_stamp_wgs(int block_if, int nch, int ntaps, int D, bool fast) {
    if (D != 10 && D != 4 && D != 3) return 0;
    if (fast) return cdiv(block_if, ft_adv(D, FT_NB)) * nch;
    return ntaps == 101 ? frontend_tiles(block_if) * nch : 0;
}

}  // namespace sdrk
