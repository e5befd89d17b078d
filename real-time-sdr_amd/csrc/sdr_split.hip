// sdr_split.hip -- the wideband splitters on MI355X (gfx950): one wide I/Q capture at W * rf_Fs into the
// R = 2 W - 1 half-overlapping u8 capture rows at rf_Fs that sdr_frontend_tuned and sdr_scan_block read
// (the definitions: include/sdr_amd.h, "wideband splitter" and "16-bit wideband splitter"). Two handles, one per
// sample width, on one scheme. All integer: every output byte, clip count and peak is defined exactly.
//
// The scheme. The work is a GEMM on the int8 matrix cores. Output sample t of every row needs the T = 16 W
// input samples from sample W t - T + 1 of the stream on: a contiguous window of K2 = 2 T components (I and Q
// interleaved), and successive windows lie 2 W components apart. The window times the [2 T x 2 R] tap matrix
//     M[2 s + 0][2 r + 0] =  g_re[r][T-1-s]     M[2 s + 0][2 r + 1] = g_im[r][T-1-s]      (the I component)
//     M[2 s + 1][2 r + 0] = -g_im[r][T-1-s]     M[2 s + 1][2 r + 1] = g_re[r][T-1-s]      (the Q component)
// gives (acc_re, acc_im) of all rows. The 14-bit entries are split exactly, e = 128 e_hi + e_lo with
// e_lo in [-64, 63] (so |e_hi| <= 64): two planes of taps for v_mfma_i32_16x16x64_i8, which recombine in int32
// (|plane sum| <= 2 T 128 64 < 2^22). -128 is an ordinary operand value.
//
// A workgroup owns SPLIT_TT consecutive outputs of one stream. It stages their windows once in LDS, one byte per
// component (from the block, or for its first T - 1 samples from the handle's history row; zeros past the
// block's end), so that output t's window starts at LDS byte 2 W (t - t0): 16-, 8- or 4-byte aligned for
// W = 8, 4, 10, read as one b128, two b64 or four b32. MFMA rows are 16 consecutive t (A = the windows), columns
// 16 of the 2 R tap columns (B = the taps, constant: a wave owns one column tile and keeps its 2 T / 64 x 2
// fragments in registers for all its time tiles). A lane then holds 4 consecutive t of one component of one
// row; neighbouring lanes hold I and Q, trade two bytes each (one DPP-sized shuffle) and store one dword of
// finished I/Q each. A row's clip counts of a wave go into one of SLOTS counters per row (by workgroup), so
// that a capture that clips throughout does not queue every wave of the grid on the same few addresses.
//
// History: two parities of the last T samples of the previous block, as they came. A block reads parity p and
// writes parity p ^ 1 (from its input, never from the history), so no workgroup overwrites what another
// still reads, whatever order they run in.
//
// The operands. k_split (int8 samples): a stream's rows are 4-byte aligned but the first window starts 2 bytes
// past a dword, so the staging shifts by two bytes (v_alignbyte); two accumulators per tile, H 128 + L in int32,
// one shift for the handle.
// k_split16 (int16 samples): a component x = 256 xh + xl (xh its signed high byte, xl its unsigned low byte) is
// staged as two int8 planes, xh as it stands and xl - 128 (the low byte with its top bit flipped), each with
// exactly the window geometry above. An input dword is one sample (I lo, I hi, Q lo, Q hi) and the first window
// starts on a sample, so the staging needs no byte shift: two samples give one dword of each plane by one
// v_perm each. Four accumulators per tile, {xh, xl - 128} x {e_hi, e_lo}, recombine as
//     acc = ((int64)(HH 128 + HL) << 8) + (LH 128 + LL) + 128 S[col],     S[col] = sum of the tap column,
// each 32-bit part below 2^25 in magnitude (128 max_col sum |e| = 2.38e7 at W = 10), while |acc| itself passes
// 2^31 for every W and stays under 2^33. Zeros (the history before block 0, the padding past a block's end) go
// through the same byte transform, so a zero sample is (0, -128) in the planes and contributes
// e (-128) + 128 e = 0. The epilogue is 64-bit: flip, the lane's row shift (read once per lane), clamp, clip
// count, max |acc|; the peak is reduced like the clip count and kept per row in slotted counters with a 64-bit
// atomicMax.
#include "stage_host.h"

#include <cmath>
#include <type_traits>
#include <vector>

namespace sdrk {
namespace {

#ifndef SPLIT_TT
#define SPLIT_TT 512
#endif
constexpr int TT = SPLIT_TT;   // outputs per workgroup (a multiple of 16 x the time groups)
constexpr int SLOTS = 64;      // partial clip and peak counters per row (summed / maxed by the reads)
constexpr int SET_RING = 4;    // pinned staging tables of sdr_split16_set_shifts in flight

struct SplitGeom {
    int N, block_iq;
};
bool split_geom(int mode, SplitGeom* g) {
    switch (mode) {
        case 0: *g = {2400, 73500}; return true;
        case 1: *g = {1440, 52920}; return true;
        case 2: *g = {2400, 80000}; return true;
        case 3: *g = {1152, 38400}; return true;
        default: return false;
    }
}
bool split_w(int W) { return W == 4 || W == 8 || W == 10; }
int split_shift_default(int W) { return W == 4 ? 14 : W == 8 ? 15 : 16; }   // (the 16-bit splitter's: 8 more)

template <int W>
struct SplitK {
    static constexpr int T = 16 * W, K2 = 2 * T, KS = K2 / 64, R = 2 * W - 1;
    static constexpr int NC = (2 * R + 15) / 16;          // column tiles (1, 2, 3)
    static constexpr int TS = NC == 1 ? 4 : 2;            // time groups of waves
    static constexpr int WAVES = NC * TS;
    static constexpr int LDS_BYTES = 2 * W * TT + K2;     // one plane: windows of TT outputs (the last ones' tails included)
    static constexpr int NDW = LDS_BYTES / 4;
    static constexpr int ALIGN = W == 8 ? 16 : W == 4 ? 8 : 4;
    static_assert(K2 % 64 == 0 && NDW % 4 == 0 && TT % (16 * TS) == 0, "tile geometry");
};
int split_ncol(int W) { return (2 * (2 * W - 1) + 15) / 16; }

typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));
template <int A>
struct V4A;   // a v4i LDS operand of known alignment only (b128, 2 x b64, 4 x b32)
template <>
struct V4A<16> {
    typedef int type __attribute__((ext_vector_type(4), aligned(16)));
};
template <>
struct V4A<8> {
    typedef int type __attribute__((ext_vector_type(4), aligned(8)));
};
template <>
struct V4A<4> {
    typedef int type __attribute__((ext_vector_type(4), aligned(4)));
};

// ---- what the two kernels share on the device (the lane decode is kept written out in both, for ISA identity)

// a wave's tap fragments of column tile ct (constant, L2-resident, lane-major)
template <int W>
__device__ __forceinline__ void split_load_taps(const v4i* __restrict__ bfrag, int ct, int lane,
                                                v4i (&BH)[SplitK<W>::KS], v4i (&BL)[SplitK<W>::KS]) {
    constexpr int KS = SplitK<W>::KS, NC = SplitK<W>::NC;
#pragma unroll
    for (int kk = 0; kk < KS; kk++) {
        BH[kk] = bfrag[((0 * NC + ct) * KS + kk) * 64 + lane];
        BL[kk] = bfrag[((1 * NC + ct) * KS + kk) * 64 + lane];
    }
}

// the pair of lanes that hold I and Q of four t (p: the lane's four finished bytes) trade two bytes each
__device__ __forceinline__ uint32_t split_trade(uint32_t p, bool even) {
    const uint32_t q = (uint32_t)__shfl_xor((int)p, 1);
    // even lane (I in p, Q in q): I0 Q0 I1 Q1; odd lane (Q in p, I in q): I2 Q2 I3 Q3
    return even ? __builtin_amdgcn_perm(q, p, 0x05010400u) : __builtin_amdgcn_perm(q, p, 0x03070206u);
}

// I/Q of two t into a row: a dword, or two halves where the rows are only 2-byte aligned
__device__ __forceinline__ void split_put(uint8_t* dst, uint32_t o, bool dwords) {
    if (dwords) {
        *reinterpret_cast<uint32_t*>(dst) = o;
    } else {
        reinterpret_cast<uint16_t*>(dst)[0] = (uint16_t)o;
        reinterpret_cast<uint16_t*>(dst)[1] = (uint16_t)(o >> 16);
    }
}

// a row's clip count of the wave (I and Q lanes, four groups of rows) in the row's first lanes
__device__ __forceinline__ unsigned split_row_clips(unsigned nclip) {
    unsigned cnt = nclip + (unsigned)__shfl_xor((int)nclip, 1);
    cnt += (unsigned)__shfl_xor((int)cnt, 16);
    cnt += (unsigned)__shfl_xor((int)cnt, 32);
    return cnt;
}

// ---- int8 samples. Grid (ceil(block_iq / TT), nwide). bfrag: [2 planes][NC][KS][64 lanes] v4i (split_fragments).
template <int W>
__global__ __launch_bounds__(64 * SplitK<W>::WAVES) void k_split(const int8_t* __restrict__ wide, size_t wide_stride,
                                                                 const uint32_t* __restrict__ hist_in,
                                                                 uint32_t* __restrict__ hist_out,
                                                                 const v4i* __restrict__ bfrag, uint8_t* __restrict__ rows,
                                                                 size_t row_stride, unsigned long long* __restrict__ clips,
                                                                 int block_iq, int shift) {
    typedef SplitK<W> G;
    constexpr int K2 = G::K2, KS = G::KS, R = G::R, NC = G::NC, TS = G::TS;
    __shared__ __attribute__((aligned(16))) int8_t win[G::LDS_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w = blockIdx.y, t0 = blockIdx.x * TT;
    const int8_t* src = wide + (size_t)w * wide_stride;
    const uint32_t* hin = hist_in + (size_t)w * (K2 / 4);
    const int limit = 2 * W * block_iq;                    // bytes in a stream's block
    // ---- stage: LDS dword i = stream bytes [s0 + 2 + 4 i, s0 + 6 + 4 i), s0 = 2 W t0 - 2 T (a multiple of 4)
    {
        const int s0 = 2 * W * t0 - K2;
        const bool interior = s0 >= 0 && s0 + 4 * G::NDW + 4 <= limit;
        uint4* dst = reinterpret_cast<uint4*>(win);
        for (int q = tid; q < G::NDW / 4; q += 64 * G::WAVES) {
            const int s = s0 + 16 * q;
            uint32_t d[5];
            if (interior) {
                const u32x4a v = *reinterpret_cast<const u32x4a*>(src + s);
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
                d[4] = *reinterpret_cast<const uint32_t*>(src + s + 16);
            } else {
#pragma unroll
                for (int j = 0; j < 5; j++) {
                    const int b = s + 4 * j;               // >= -2 T
                    d[j] = b < 0 ? hin[(b + K2) >> 2] : b < limit ? *reinterpret_cast<const uint32_t*>(src + b) : 0u;
                }
            }
            dst[q] = uint4{__builtin_amdgcn_alignbyte(d[1], d[0], 2), __builtin_amdgcn_alignbyte(d[2], d[1], 2),
                           __builtin_amdgcn_alignbyte(d[3], d[2], 2), __builtin_amdgcn_alignbyte(d[4], d[3], 2)};
        }
        // the next block's history: this block's last T samples (block_iq >= T in every mode)
        if (blockIdx.x == 0 && tid < K2 / 4)
            hist_out[(size_t)w * (K2 / 4) + tid] = *reinterpret_cast<const uint32_t*>(src + limit - K2 + 4 * tid);
    }
    const int ct = wave % NC, ts = wave / NC;
    v4i BH[KS], BL[KS];
    split_load_taps<W>(bfrag, ct, lane, BH, BL);
    __syncthreads();
    const int n = lane & 15, g = lane >> 4;
    const int c = 16 * ct + n, r = c >> 1;
    const bool valid = c < 2 * R;
    const bool kodd = ((r - (W - 1)) & 1) != 0;
    const bool even = (lane & 1) == 0;
    const bool dwords = ((reinterpret_cast<uintptr_t>(rows) | row_stride) & 3) == 0;   // else 2-byte aligned rows
    uint8_t* orow = rows + ((size_t)w * R + (valid ? r : 0)) * row_stride;
    const int half = 1 << (shift - 1);
    unsigned nclip = 0;
    for (int tile = ts; tile < TT / 16; tile += TS) {
        const int tb = t0 + 16 * tile;
        if (tb >= block_iq) break;
        v4i H = {0, 0, 0, 0}, L = {0, 0, 0, 0};
        const int8_t* wp = win + 2 * W * (16 * tile + n) + 16 * g;
#pragma unroll
        for (int kk = 0; kk < KS; kk++) {
            const v4i a = *reinterpret_cast<const typename V4A<G::ALIGN>::type*>(wp + 64 * kk);
            H = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, BH[kk], H, 0, 0, 0);
            L = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, BL[kk], L, 0, 0, 0);
        }
        // rows of the C tile: t = tb + 4 g + j (tb and 4 g even: j odd is t odd)
        uint32_t p = 0;
        unsigned over = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int acc = H[j] * 128 + L[j];
            if ((j & 1) && kodd) acc = -acc;
            const int v = 128 + ((acc + half) >> shift);
            over += (v < 0 || v > 255) ? 1u : 0u;
            p |= (uint32_t)min(max(v, 0), 255) << (8 * j);
        }
        const int t4 = tb + 4 * g;                         // block_iq is a multiple of 4: all four t or none
        if (valid && t4 < block_iq) nclip += over;
        const uint32_t o = split_trade(p, even);
        if (valid && t4 < block_iq) split_put(orow + 2 * (size_t)t4 + (even ? 0 : 4), o, dwords);
    }
    // one atomic per row and wave
    const unsigned cnt = split_row_clips(nclip);
    if (valid && even && lane < 16 && cnt)
        atomicAdd(clips + ((size_t)w * R + r) * SLOTS + (blockIdx.x % SLOTS), (unsigned long long)cnt);
}

// ---- int16 samples
// two samples (I lo, I hi, Q lo, Q hi each) -> the high-byte plane's dword and the low-byte plane's (xl - 128)
__device__ __forceinline__ uint32_t plane_hi(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07050301u); }
__device__ __forceinline__ uint32_t plane_lo(uint32_t a, uint32_t b) {
    return __builtin_amdgcn_perm(b, a, 0x06040200u) ^ 0x80808080u;
}

// Grid (ceil(block_iq / TT), nwide). wide: samples as dwords, wide_stride in dwords. bfrag: as k_split's;
// colsum: [16 NC] (0 past 2 R); shifts: [nwide][R]; clips, peaks: [nwide][R][SLOTS].
template <int W>
__global__ __launch_bounds__(64 * SplitK<W>::WAVES) void k_split16(
    const uint32_t* __restrict__ wide, size_t wide_stride, const uint32_t* __restrict__ hist_in,
    uint32_t* __restrict__ hist_out, const v4i* __restrict__ bfrag, const int* __restrict__ colsum,
    const int* __restrict__ shifts, uint8_t* __restrict__ rows, size_t row_stride,
    unsigned long long* __restrict__ clips, unsigned long long* __restrict__ peaks, int block_iq) {
    typedef SplitK<W> G;
    constexpr int T = G::T, KS = G::KS, R = G::R, NC = G::NC, TS = G::TS;
    static_assert(T <= 64 * G::WAVES, "one thread per history dword");
    __shared__ __attribute__((aligned(16))) int8_t win_h[G::LDS_BYTES];
    __shared__ __attribute__((aligned(16))) int8_t win_l[G::LDS_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w = blockIdx.y, t0 = blockIdx.x * TT;
    const uint32_t* src = wide + (size_t)w * wide_stride;
    const uint32_t* hin = hist_in + (size_t)w * T;
    const int limit = W * block_iq;                        // samples in a stream's block
    // ---- stage: dword i of each plane = samples p0 + 2 i and p0 + 2 i + 1, p0 = W t0 - T + 1 (the first window's)
    {
        const int p0 = W * t0 - T + 1;
        const bool interior = p0 >= 0 && p0 + 2 * G::NDW <= limit;
        uint4* dh = reinterpret_cast<uint4*>(win_h);
        uint4* dl = reinterpret_cast<uint4*>(win_l);
        for (int q = tid; q < G::NDW / 4; q += 64 * G::WAVES) {
            const int p = p0 + 8 * q;
            uint32_t d[8];
            if (interior) {
                const u32x4a u = *reinterpret_cast<const u32x4a*>(src + p);
                const u32x4a v = *reinterpret_cast<const u32x4a*>(src + p + 4);
                d[0] = u.x; d[1] = u.y; d[2] = u.z; d[3] = u.w;
                d[4] = v.x; d[5] = v.y; d[6] = v.z; d[7] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int b = p + j;                   // >= -(T - 1)
                    d[j] = b < 0 ? hin[b + T] : b < limit ? src[b] : 0u;
                }
            }
            dh[q] = uint4{plane_hi(d[0], d[1]), plane_hi(d[2], d[3]), plane_hi(d[4], d[5]), plane_hi(d[6], d[7])};
            dl[q] = uint4{plane_lo(d[0], d[1]), plane_lo(d[2], d[3]), plane_lo(d[4], d[5]), plane_lo(d[6], d[7])};
        }
        // the next block's history: this block's last T samples (block_iq >= T in every mode)
        if (blockIdx.x == 0 && tid < T) hist_out[(size_t)w * T + tid] = src[limit - T + tid];
    }
    const int ct = wave % NC, ts = wave / NC;
    v4i BH[KS], BL[KS];
    split_load_taps<W>(bfrag, ct, lane, BH, BL);
    const int n = lane & 15, g = lane >> 4;
    const int c = 16 * ct + n, r = c >> 1;
    const bool valid = c < 2 * R;
    const bool kodd = ((r - (W - 1)) & 1) != 0;
    const bool even = (lane & 1) == 0;
    const bool dwords = ((reinterpret_cast<uintptr_t>(rows) | row_stride) & 3) == 0;   // else 2-byte aligned rows
    const size_t orow_i = (size_t)w * R + (valid ? r : 0);
    uint8_t* orow = rows + orow_i * row_stride;
    const int shift = shifts[orow_i];
    const long long half = 1LL << (shift - 1);
    const long long bias = 128LL * colsum[c];
    __syncthreads();
    unsigned nclip = 0;
    long long peak = 0;
    for (int tile = ts; tile < TT / 16; tile += TS) {
        const int tb = t0 + 16 * tile;
        if (tb >= block_iq) break;
        v4i HH = {0, 0, 0, 0}, HL = {0, 0, 0, 0}, LH = {0, 0, 0, 0}, LL = {0, 0, 0, 0};
        const int off = 2 * W * (16 * tile + n) + 16 * g;
#pragma unroll
        for (int kk = 0; kk < KS; kk++) {
            const v4i ah = *reinterpret_cast<const typename V4A<G::ALIGN>::type*>(win_h + off + 64 * kk);
            const v4i al = *reinterpret_cast<const typename V4A<G::ALIGN>::type*>(win_l + off + 64 * kk);
            HH = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, BH[kk], HH, 0, 0, 0);
            HL = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, BL[kk], HL, 0, 0, 0);
            LH = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, BH[kk], LH, 0, 0, 0);
            LL = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, BL[kk], LL, 0, 0, 0);
        }
        // rows of the C tile: t = tb + 4 g + j (tb and 4 g even: j odd is t odd)
        uint32_t p = 0;
        unsigned over = 0;
        long long big = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            long long acc = ((long long)(HH[j] * 128 + HL[j]) << 8) + (long long)(LH[j] * 128 + LL[j]) + bias;
            if ((j & 1) && kodd) acc = -acc;
            const long long mag = acc < 0 ? -acc : acc;
            big = mag > big ? mag : big;
            const long long v = 128 + ((acc + half) >> shift);
            over += (v < 0 || v > 255) ? 1u : 0u;
            p |= (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v) << (8 * j);
        }
        const int t4 = tb + 4 * g;                         // block_iq is a multiple of 4: all four t or none
        if (valid && t4 < block_iq) {
            nclip += over;
            peak = big > peak ? big : peak;
        }
        const uint32_t o = split_trade(p, even);
        if (valid && t4 < block_iq) split_put(orow + 2 * (size_t)t4 + (even ? 0 : 4), o, dwords);
    }
    // the row's peak of the wave as its clip count, then one atomic each per row and wave
    const unsigned cnt = split_row_clips(nclip);
    long long o1 = __shfl_xor(peak, 1);
    peak = o1 > peak ? o1 : peak;
    o1 = __shfl_xor(peak, 16);
    peak = o1 > peak ? o1 : peak;
    o1 = __shfl_xor(peak, 32);
    peak = o1 > peak ? o1 : peak;
    if (valid && even && lane < 16) {
        const size_t slot = ((size_t)w * R + r) * SLOTS + (blockIdx.x % SLOTS);
        if (cnt) atomicAdd(clips + slot, (unsigned long long)cnt);
        if (peak) atomicMax(peaks + slot, (unsigned long long)peak);
    }
}

// g[r][m] = (re, im), the definition's table
void split_taps(int W, int16_t* g) {
    const int T = 16 * W, R = 2 * W - 1;
    const double pi = 3.14159265358979323846;
    for (int r = 0; r < R; r++) {
        const int k = r - (W - 1);
        for (int m = 0; m < T; m++) {
            const double u = (double)m - (double)(T - 1) / 2.0;
            const double x = u / (double)W;
            const double sinc = std::sin(pi * x) / (pi * x);
            const double win = 0.42 - 0.5 * std::cos(2.0 * pi * ((double)m + 0.5) / (double)T) +
                               0.08 * std::cos(4.0 * pi * ((double)m + 0.5) / (double)T);
            const double h = sinc * win;
            int a = (k * (2 * m - T + 1)) % (4 * W);
            if (a < 0) a += 4 * W;
            const double th = pi * (double)a / (double)(2 * W);
            g[2 * (r * T + m)] = (int16_t)std::rint(8191.0 * h * std::cos(th));
            g[2 * (r * T + m) + 1] = (int16_t)std::rint(8191.0 * h * std::sin(th));
        }
    }
}

// The tap matrix M as the MFMA's B fragments: lane l of fragment (plane, ct, kk) holds
// M[64 kk + 16 (l >> 4) + j][16 ct + (l & 15)], j < 16, as int8 (columns past 2 R are zero); and, where asked
// for, the column sums S[16 NC].
std::vector<int8_t> split_fragments(int W, std::vector<int>* colsum = nullptr) {
    const int T = 16 * W, R = 2 * W - 1, KS = 2 * T / 64, NC = split_ncol(W);
    std::vector<int16_t> g((size_t)2 * R * T);
    split_taps(W, g.data());
    std::vector<int8_t> f((size_t)2 * NC * KS * 64 * 16, 0);
    if (colsum) *colsum = std::vector<int>((size_t)16 * NC, 0);
    for (int ct = 0; ct < NC; ct++)
        for (int kk = 0; kk < KS; kk++)
            for (int l = 0; l < 64; l++)
                for (int j = 0; j < 16; j++) {
                    const int row = 64 * kk + 16 * (l >> 4) + j, col = 16 * ct + (l & 15);
                    if (col >= 2 * R) continue;
                    const int s = row >> 1, q = row & 1, r = col >> 1, im = col & 1;
                    const int m = T - 1 - s;
                    const int gre = g[2 * (r * T + m)], gim = g[2 * (r * T + m) + 1];
                    const int e = im ? (q ? gre : gim) : (q ? -gim : gre);
                    const int lo = ((e + 64) & 127) - 64, hi = (e - lo) / 128;
                    f[((((size_t)0 * NC + ct) * KS + kk) * 64 + l) * 16 + j] = (int8_t)hi;
                    f[((((size_t)1 * NC + ct) * KS + kk) * 64 + l) * 16 + j] = (int8_t)lo;
                    if (colsum) (*colsum)[col] += e;
                }
    return f;
}

// ---- what the two handles share on the host

// the part both handles have. hist: [2][nwide][T] samples (2 T bytes or T dwords each)
struct SplitCore {
    int device = 0, mode = 0, W = 0, nwide = 0;
    SplitGeom g{};
    int parity = 0;                          // the history row the next block reads
    uint32_t* hist = nullptr;
    v4i* bfrag = nullptr;
    unsigned long long* clips = nullptr;     // [nwide][R][SLOTS]
    size_t rows() const { return (size_t)nwide * (2 * W - 1); }
    size_t slot_bytes() const { return rows() * SLOTS * sizeof(unsigned long long); }
};

// the splitters' rule for their arguments; `who` names the caller in the text. *shift <= 0 becomes `dflt`,
// the shifts go up to `top`
int split_rule(const char* who, int mode, int W, int nwide, int* shift, int dflt, int top, SplitGeom* g) {
    if (!split_geom(mode, g)) return fail(SDR_E_INVALID, "%s: mode %d not in 0..3", who, mode);
    if (!split_w(W)) return fail(SDR_E_INVALID, "%s: W %d not 4, 8 or 10", who, W);
    if (nwide < 1 || nwide > 4096) return fail(SDR_E_INVALID, "%s: nwide %d outside [1, 4096]", who, nwide);
    if (*shift <= 0) *shift = split_shift_default(W) + dflt;
    if (*shift > top) return fail(SDR_E_INVALID, "%s: shift %d outside [1, %d]", who, *shift, top);
    return SDR_OK;
}

// a block call's rule for its rows; sample: bytes of an input sample (2 or 4)
int split_block_rule(const char* who, const SplitCore* s, const void* wide, size_t wide_stride, const void* rows,
                     size_t row_stride, int sample) {
    const size_t wide_bytes = (size_t)sample * s->W * s->g.block_iq;
    if (wide_stride < wide_bytes || (wide_stride & 3) || (reinterpret_cast<uintptr_t>(wide) & 3))
        return fail(SDR_E_INVALID, "%s: wide_stride %zu < %d*W*block_iq %zu, or not 4-byte aligned", who, wide_stride,
                    sample, wide_bytes);
    if (row_stride < (size_t)2 * s->g.block_iq || (row_stride & 1) || (reinterpret_cast<uintptr_t>(rows) & 1))
        return fail(SDR_E_INVALID, "%s: row_stride %zu < 2*block_iq %d or misaligned", who, row_stride,
                    2 * s->g.block_iq);
    return SDR_OK;
}

// a create's common links: the arguments into the handle, its three buffers (hist of hist_bytes), the fragments
// up, history and clip counters zero
void split_core_init(hipError_t& e, SplitCore* s, int mode, int W, int nwide, const SplitGeom& g, size_t hist_bytes,
                     const std::vector<int8_t>& f) {
    s->mode = mode;
    s->W = W;
    s->nwide = nwide;
    s->g = g;
    dev_alloc(e, &s->hist, hist_bytes);
    dev_alloc(e, &s->bfrag, f.size());
    dev_alloc(e, &s->clips, s->slot_bytes());
    if (e == hipSuccess) e = hipMemcpy(s->bfrag, f.data(), f.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(s->hist, 0, hist_bytes);
    if (e == hipSuccess) e = hipMemset(s->clips, 0, s->slot_bytes());
}

// f(W as a constant) for the handle's W
template <typename F>
void split_with_w(int W, F f) {
    switch (W) {
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        default: f(std::integral_constant<int, 10>{}); break;
    }
}

// the history parity a block reads and the one it writes, of `dwords` each
void split_history(const SplitCore* s, size_t dwords, const uint32_t** hin, uint32_t** hout) {
    *hin = s->hist + (size_t)s->parity * dwords;
    *hout = s->hist + (size_t)(s->parity ^ 1) * dwords;
}

// out[i] = the sum (or the max) of row i's SLOTS counters: the copy, a clearing memset behind it on the stream
// where asked for, and one wait for both
int split_read_slots(const SplitCore* s, unsigned long long* dev, long long* out, bool max, bool clear, hipStream_t st) {
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = s->rows();
    std::vector<unsigned long long> part(n * SLOTS);
    HIP_TRY(hipMemcpyAsync(part.data(), dev, s->slot_bytes(), hipMemcpyDeviceToHost, st));
    if (clear) HIP_TRY(hipMemsetAsync(dev, 0, s->slot_bytes(), st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; i++) {
        unsigned long long v = 0;
        for (int k = 0; k < SLOTS; k++) {
            const unsigned long long x = part[i * SLOTS + k];
            v = max ? (x > v ? x : v) : v + x;
        }
        out[i] = (long long)v;
    }
    return SDR_OK;
}

}  // namespace
}  // namespace sdrk

using namespace sdrk;

struct sdr_split : SplitCore {
    int shift = 0;
};

struct sdr_split16 : SplitCore {
    int* colsum = nullptr;                   // [16 NC]
    int* shifts = nullptr;                   // [nwide][R]
    unsigned long long* peaks = nullptr;     // [nwide][R][SLOTS]
    // sdr_split16_set_shifts: pinned tables [SET_RING][nwide R] the copies read, and an event behind each copy
    int* stage = nullptr;
    hipEvent_t staged[SET_RING] = {};
    int next = 0;
};

extern "C" {

int sdr_split_geometry(int mode, int W, int* rows, int* taps, int* wide_iq, int* half_khz, int* shift_default) {
    SplitGeom g;
    if (!split_geom(mode, &g)) return fail(SDR_E_INVALID, "split_geometry: mode %d not in 0..3", mode);
    if (!split_w(W)) return fail(SDR_E_INVALID, "split_geometry: W %d not 4, 8 or 10", W);
    if (rows) *rows = 2 * W - 1;
    if (taps) *taps = 16 * W;
    if (wide_iq) *wide_iq = W * g.block_iq;
    if (half_khz) *half_khz = g.N / 2;
    if (shift_default) *shift_default = split_shift_default(W);
    return SDR_OK;
}

int sdr_split_taps(int W, int16_t* g, int max_pairs, int* n) {
    if (!split_w(W) || !n) return fail(SDR_E_INVALID, "split_taps: W %d not 4, 8 or 10, or null n", W);
    const int total = (2 * W - 1) * 16 * W;
    if (g && max_pairs < total) return fail(SDR_E_INVALID, "split_taps: room for %d of %d pairs", max_pairs, total);
    *n = total;
    if (g) split_taps(W, g);
    return SDR_OK;
}

// ---- the int8 handle

int sdr_split_check(int mode, int W, int nwide, int shift) {
    SplitGeom g;
    return split_rule("split_check", mode, W, nwide, &shift, 0, 24, &g);
}

int sdr_split_create(sdr_split** out, int device, int mode, int W, int nwide, int shift) {
    if (!out) return fail(SDR_E_INVALID, "split_create: out is NULL");
    *out = nullptr;
    SplitGeom g;
    if (const int r = split_rule("split_create", mode, W, nwide, &shift, 0, 24, &g)) return r;
    const std::vector<int8_t> f = split_fragments(W);
    sdr_split* s = nullptr;
    if (const int r = create_begin(&s, device, "split_create")) return r;
    s->shift = shift;
    hipError_t e = hipSuccess;
    split_core_init(e, s, mode, W, nwide, g, (size_t)2 * nwide * 32 * W, f);
    return create_done(e, s, out, sdr_split_destroy, "split_create");
}

int sdr_split_destroy(sdr_split* s) {
    if (!s) return fail(SDR_E_INVALID, "split_destroy: null splitter");
    return destroy_handle(s, {s->hist, s->bfrag, s->clips});
}

int sdr_split_reset(sdr_split* s, void* stream) {
    if (!s) return fail(SDR_E_INVALID, "split_reset: null splitter");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemsetAsync(s->hist, 0, (size_t)2 * s->nwide * 32 * s->W, S(stream)));
    HIP_TRY(hipMemsetAsync(s->clips, 0, s->slot_bytes(), S(stream)));
    s->parity = 0;
    return SDR_OK;
}

int sdr_split_block(sdr_split* s, const int8_t* wide, size_t wide_stride, uint8_t* rows, size_t row_stride,
                    void* stream) {
    if (!s || !wide || !rows) return fail(SDR_E_INVALID, "split_block: null argument");
    if (const int r = split_block_rule("split_block", s, wide, wide_stride, rows, row_stride, 2)) return r;
    HIP_TRY(hipSetDevice(s->device));
    const uint32_t* hin;
    uint32_t* hout;
    split_history(s, (size_t)s->nwide * 8 * s->W, &hin, &hout);
    split_with_w(s->W, [&](auto w) {
        constexpr int W = decltype(w)::value;
        hipLaunchKernelGGL(k_split<W>, dim3(cdiv(s->g.block_iq, TT), s->nwide), dim3(64 * SplitK<W>::WAVES), 0, S(stream),
                           wide, wide_stride, hin, hout, s->bfrag, rows, row_stride, s->clips, s->g.block_iq, s->shift);
    });
    LAUNCH_CHECK();
    s->parity ^= 1;
    return SDR_OK;
}

int sdr_split_clips(sdr_split* s, long long* clips, void* stream) {
    if (!s || !clips) return fail(SDR_E_INVALID, "split_clips: null argument");
    return split_read_slots(s, s->clips, clips, false, false, S(stream));
}

// ---- the int16 handle

int sdr_split16_shift_for(long long peak, int target, int W) {
    if (!split_w(W)) return fail(SDR_E_INVALID, "split16_shift_for: W %d not 4, 8 or 10", W);
    if (target < 1 || target > 127) return fail(SDR_E_INVALID, "split16_shift_for: target %d outside [1, 127]", target);
    if (peak < 0) return fail(SDR_E_INVALID, "split16_shift_for: negative peak");
    if (peak == 0) return split_shift_default(W) + 8;
    for (int s = 1; s < 33; s++)
        if (((peak + (1LL << (s - 1))) >> s) <= target) return s;
    return 33;
}

int sdr_split16_check(int mode, int W, int nwide, int shift) {
    SplitGeom g;
    return split_rule("split16_check", mode, W, nwide, &shift, 8, 33, &g);
}

int sdr_split16_create(sdr_split16** out, int device, int mode, int W, int nwide, int shift) {
    if (!out) return fail(SDR_E_INVALID, "split16_create: out is NULL");
    *out = nullptr;
    SplitGeom g;
    if (const int r = split_rule("split16_create", mode, W, nwide, &shift, 8, 33, &g)) return r;
    std::vector<int> cs;
    const std::vector<int8_t> f = split_fragments(W, &cs);
    sdr_split16* s = nullptr;
    if (const int r = create_begin(&s, device, "split16_create")) return r;
    hipError_t e = hipSuccess;
    split_core_init(e, s, mode, W, nwide, g, (size_t)2 * nwide * 16 * W * sizeof(uint32_t), f);
    const size_t nr = s->rows();
    const std::vector<int> sh(nr, shift);
    dev_alloc(e, &s->colsum, cs.size() * sizeof(int));
    dev_alloc(e, &s->shifts, nr * sizeof(int));
    dev_alloc(e, &s->peaks, s->slot_bytes());
    if (e == hipSuccess) e = hipHostMalloc((void**)&s->stage, SET_RING * nr * sizeof(int), hipHostMallocDefault);
    for (int k = 0; k < SET_RING; k++)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->staged[k], hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemcpy(s->colsum, cs.data(), cs.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->shifts, sh.data(), nr * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(s->peaks, 0, s->slot_bytes());
    return create_done(e, s, out, sdr_split16_destroy, "split16_create");
}

int sdr_split16_destroy(sdr_split16* s) {
    if (!s) return fail(SDR_E_INVALID, "split16_destroy: null splitter");
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    for (hipEvent_t ev : s->staged)
        if (ev) (void)hipEventDestroy(ev);
    if (s->stage) (void)hipHostFree(s->stage);
    return destroy_handle(s, {s->hist, s->bfrag, s->colsum, s->shifts, s->clips, s->peaks});
}

int sdr_split16_reset(sdr_split16* s, void* stream) {
    if (!s) return fail(SDR_E_INVALID, "split16_reset: null splitter");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemsetAsync(s->hist, 0, (size_t)2 * s->nwide * 16 * s->W * sizeof(uint32_t), S(stream)));
    HIP_TRY(hipMemsetAsync(s->clips, 0, s->slot_bytes(), S(stream)));
    HIP_TRY(hipMemsetAsync(s->peaks, 0, s->slot_bytes(), S(stream)));
    s->parity = 0;
    return SDR_OK;
}

int sdr_split16_set_shifts(sdr_split16* s, const int* shifts, void* stream) {
    if (!s || !shifts) return fail(SDR_E_INVALID, "split16_set_shifts: null argument");
    const size_t nr = s->rows();
    for (size_t i = 0; i < nr; i++)
        if (shifts[i] < 1 || shifts[i] > 33)
            return fail(SDR_E_INVALID, "split16_set_shifts: shift %d of row %zu outside [1, 33]", shifts[i], i);
    HIP_TRY(hipSetDevice(s->device));
    // the copy reads a pinned table of the handle's, so the caller's may go at once; a table is reused only
    // after the copy that read it last (SET_RING calls ago) has run
    const int k = s->next;
    HIP_TRY(hipEventSynchronize(s->staged[k]));
    int* tab = s->stage + (size_t)k * nr;
    for (size_t i = 0; i < nr; i++) tab[i] = shifts[i];
    HIP_TRY(hipMemcpyAsync(s->shifts, tab, nr * sizeof(int), hipMemcpyHostToDevice, S(stream)));
    HIP_TRY(hipEventRecord(s->staged[k], S(stream)));
    s->next = (k + 1) % SET_RING;
    return SDR_OK;
}

int sdr_split16_block(sdr_split16* s, const int16_t* wide, size_t wide_stride, uint8_t* rows, size_t row_stride,
                      void* stream) {
    if (!s || !wide || !rows) return fail(SDR_E_INVALID, "split16_block: null argument");
    if (const int r = split_block_rule("split16_block", s, wide, wide_stride, rows, row_stride, 4)) return r;
    HIP_TRY(hipSetDevice(s->device));
    const uint32_t* hin;
    uint32_t* hout;
    split_history(s, (size_t)s->nwide * 16 * s->W, &hin, &hout);
    split_with_w(s->W, [&](auto w) {
        constexpr int W = decltype(w)::value;
        hipLaunchKernelGGL(k_split16<W>, dim3(cdiv(s->g.block_iq, TT), s->nwide), dim3(64 * SplitK<W>::WAVES), 0, S(stream),
                           reinterpret_cast<const uint32_t*>(wide), wide_stride / 4, hin, hout, s->bfrag, s->colsum,
                           s->shifts, rows, row_stride, s->clips, s->peaks, s->g.block_iq);
    });
    LAUNCH_CHECK();
    s->parity ^= 1;
    return SDR_OK;
}

int sdr_split16_clips(sdr_split16* s, long long* clips, void* stream) {
    if (!s || !clips) return fail(SDR_E_INVALID, "split16_clips: null argument");
    return split_read_slots(s, s->clips, clips, false, false, S(stream));
}

int sdr_split16_peaks(sdr_split16* s, long long* peaks, int clear, void* stream) {
    if (!s || !peaks) return fail(SDR_E_INVALID, "split16_peaks: null argument");
    return split_read_slots(s, s->peaks, peaks, true, clear != 0, S(stream));
}

}  // extern "C"
