// sdr_split.hip -- wideband splitter on MI355X (gfx950): one wide s8 I/Q capture at W * rf_Fs into the
// R = 2 W - 1 half-overlapping u8 capture rows at rf_Fs that sdr_frontend_tuned and sdr_scan_block read
// (the definition: include/sdr_amd.h, "wideband splitter"). All integer: every output byte and every
// clip count is defined exactly.
//
// The work is a GEMM on the int8 matrix cores. Output sample t of every row needs the 2 T input bytes
// from byte 2 (W t - T + 1) of the stream on (T = 16 W taps, I and Q interleaved): a contiguous window,
// and successive windows lie 2 W bytes apart. The window times the [2 T x 2 R] tap matrix
//     M[2 s + 0][2 r + 0] =  g_re[r][T-1-s]     M[2 s + 0][2 r + 1] = g_im[r][T-1-s]      (the I byte)
//     M[2 s + 1][2 r + 0] = -g_im[r][T-1-s]     M[2 s + 1][2 r + 1] = g_re[r][T-1-s]      (the Q byte)
// gives (acc_re, acc_im) of all rows. The 14-bit entries are split exactly, e = 128 e_hi + e_lo with
// e_lo in [-64, 63] (so |e_hi| <= 64): two v_mfma_i32_16x16x64_i8 planes that recombine in int32
// (|plane sum| <= 2 T 128 64 < 2^22). -128 is an ordinary operand value.
//
// A workgroup owns SPLIT_TT consecutive outputs of one stream. It stages their 2 W SPLIT_TT + 2 T bytes
// once in LDS (from the block, or for its first T - 1 samples from the handle's history row; zeros past
// the block's end). The stream's rows are 4-byte aligned but the first window starts 2 bytes past a
// dword, so the staging shifts by two bytes (v_alignbyte) and every window then starts at LDS byte
// 2 W (t - t0): 16-, 8- or 4-byte aligned for W = 8, 4, 10, read as one b128, two b64 or four b32.
// MFMA rows are 16 consecutive t (A = the windows), columns 16 of the 2 R tap columns (B = the taps,
// constant: a wave owns one column tile and keeps its 2 T / 64 x 2 fragments in registers for all its
// time tiles). A lane then holds 4 consecutive t of one component of one row; neighbouring lanes hold
// I and Q, trade two bytes each (one DPP-sized shuffle) and store one dword of finished I/Q each.
//
// History: [2][nwide][2 T] bytes, the last T samples of the previous block. A block reads parity p and
// writes parity p ^ 1 (from its input, never from the history), so no workgroup overwrites what
// another still reads, whatever order they run in.
#include "stage_host.h"

#include <cmath>
#include <vector>

namespace sdrk {
namespace {

#ifndef SPLIT_TT
#define SPLIT_TT 512
#endif
constexpr int TT = SPLIT_TT;   // outputs per workgroup (a multiple of 16 x the time groups)
constexpr int CLIP_SLOTS = 64; // partial clip counters per row (summed by sdr_split_clips)

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
int split_shift_default(int W) { return W == 4 ? 14 : W == 8 ? 15 : 16; }

template <int W>
struct SplitK {
    static constexpr int T = 16 * W, K2 = 2 * T, KS = K2 / 64, R = 2 * W - 1;
    static constexpr int NC = (2 * R + 15) / 16;          // column tiles (1, 2, 3)
    static constexpr int TS = NC == 1 ? 4 : 2;            // time groups of waves
    static constexpr int WAVES = NC * TS;
    static constexpr int LDS_BYTES = 2 * W * TT + K2;     // windows of TT outputs (the last ones' tails included)
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

// Grid (ceil(block_iq / TT), nwide). bfrag: [2 planes][NC][KS][64 lanes] v4i (split_fragments).
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
    // ---- this wave's tap fragments (constant, L2-resident, lane-major)
    const int ct = wave % NC, ts = wave / NC;
    v4i BH[KS], BL[KS];
#pragma unroll
    for (int kk = 0; kk < KS; kk++) {
        BH[kk] = bfrag[((0 * NC + ct) * KS + kk) * 64 + lane];
        BL[kk] = bfrag[((1 * NC + ct) * KS + kk) * 64 + lane];
    }
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
        const uint32_t q = (uint32_t)__shfl_xor((int)p, 1);
        // even lane (I in p, Q in q): I0 Q0 I1 Q1; odd lane (Q in p, I in q): I2 Q2 I3 Q3
        const uint32_t o = even ? __builtin_amdgcn_perm(q, p, 0x05010400u) : __builtin_amdgcn_perm(q, p, 0x03070206u);
        if (valid && t4 < block_iq) {
            uint8_t* dst = orow + 2 * (size_t)t4 + (even ? 0 : 4);
            if (dwords) {
                *reinterpret_cast<uint32_t*>(dst) = o;
            } else {
                reinterpret_cast<uint16_t*>(dst)[0] = (uint16_t)o;
                reinterpret_cast<uint16_t*>(dst)[1] = (uint16_t)(o >> 16);
            }
        }
    }
    // a row's counts of the wave (I and Q lanes, four groups of rows) in one lane, then one atomic per row
    // and wave into one of CLIP_SLOTS counters (by workgroup), so that a capture that clips throughout does
    // not queue every wave of the grid on the same few addresses
    unsigned cnt = nclip + (unsigned)__shfl_xor((int)nclip, 1);
    cnt += (unsigned)__shfl_xor((int)cnt, 16);
    cnt += (unsigned)__shfl_xor((int)cnt, 32);
    if (valid && even && lane < 16 && cnt)
        atomicAdd(clips + ((size_t)w * R + r) * CLIP_SLOTS + (blockIdx.x % CLIP_SLOTS), (unsigned long long)cnt);
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
// M[64 kk + 16 (l >> 4) + j][16 ct + (l & 15)], j < 16, as int8 (columns past 2 R are zero).
std::vector<int8_t> split_fragments(int W) {
    const int T = 16 * W, R = 2 * W - 1, KS = 2 * T / 64, NC = split_ncol(W);
    std::vector<int16_t> g((size_t)2 * R * T);
    split_taps(W, g.data());
    std::vector<int8_t> f((size_t)2 * NC * KS * 64 * 16, 0);
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
                }
    return f;
}

}  // namespace
}  // namespace sdrk

using namespace sdrk;

struct sdr_split {
    int device = 0, mode = 0, W = 0, nwide = 0, shift = 0;
    SplitGeom g{};
    int parity = 0;                          // the history row the next block reads
    uint32_t* hist = nullptr;                // [2][nwide][2 T / 4]
    v4i* bfrag = nullptr;
    unsigned long long* clips = nullptr;     // [nwide][R][CLIP_SLOTS]
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

// the splitter's rule for its arguments; `who` names the caller in the text. *shift <= 0 becomes W's default
static int split_rule(const char* who, int mode, int W, int nwide, int* shift, SplitGeom* g) {
    if (!split_geom(mode, g)) return fail(SDR_E_INVALID, "%s: mode %d not in 0..3", who, mode);
    if (!split_w(W)) return fail(SDR_E_INVALID, "%s: W %d not 4, 8 or 10", who, W);
    if (nwide < 1 || nwide > 4096) return fail(SDR_E_INVALID, "%s: nwide %d outside [1, 4096]", who, nwide);
    if (*shift <= 0) *shift = split_shift_default(W);
    if (*shift > 24) return fail(SDR_E_INVALID, "%s: shift %d outside [1, 24]", who, *shift);
    return SDR_OK;
}

int sdr_split_check(int mode, int W, int nwide, int shift) {
    SplitGeom g;
    return split_rule("split_check", mode, W, nwide, &shift, &g);
}

int sdr_split_create(sdr_split** out, int device, int mode, int W, int nwide, int shift) {
    if (!out) return fail(SDR_E_INVALID, "split_create: out is NULL");
    *out = nullptr;
    SplitGeom g;
    if (const int r = split_rule("split_create", mode, W, nwide, &shift, &g)) return r;
    sdr_split* s = nullptr;
    if (const int r = create_begin(&s, device, "split_create")) return r;
    s->mode = mode;
    s->W = W;
    s->nwide = nwide;
    s->shift = shift;
    s->g = g;
    const std::vector<int8_t> f = split_fragments(W);
    const size_t nh = (size_t)2 * nwide * 32 * W, nc = (size_t)nwide * (2 * W - 1) * CLIP_SLOTS;
    hipError_t e = hipSuccess;
    dev_alloc(e, &s->hist, nh);
    dev_alloc(e, &s->bfrag, f.size());
    dev_alloc(e, &s->clips, nc * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemcpy(s->bfrag, f.data(), f.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(s->hist, 0, nh);
    if (e == hipSuccess) e = hipMemset(s->clips, 0, nc * sizeof(unsigned long long));
    return create_done(e, s, out, sdr_split_destroy, "split_create");
}

int sdr_split_destroy(sdr_split* s) {
    if (!s) return fail(SDR_E_INVALID, "split_destroy: null splitter");
    return destroy_handle(s, {s->hist, s->bfrag, s->clips});
}

int sdr_split_reset(sdr_split* s, void* stream) {
    if (!s) return fail(SDR_E_INVALID, "split_reset: null splitter");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemsetAsync(s->hist, 0, (size_t)2 * s->nwide * 32 * s->W, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(s->clips, 0, (size_t)s->nwide * (2 * s->W - 1) * CLIP_SLOTS * sizeof(unsigned long long),
                           (hipStream_t)stream));
    s->parity = 0;
    return SDR_OK;
}

int sdr_split_block(sdr_split* s, const int8_t* wide, size_t wide_stride, uint8_t* rows, size_t row_stride,
                    void* stream) {
    if (!s || !wide || !rows) return fail(SDR_E_INVALID, "split_block: null argument");
    const size_t wide_bytes = (size_t)2 * s->W * s->g.block_iq;
    if (wide_stride < wide_bytes || (wide_stride & 3) || (reinterpret_cast<uintptr_t>(wide) & 3))
        return fail(SDR_E_INVALID, "split_block: wide_stride %zu < 2*W*block_iq %zu, or not 4-byte aligned", wide_stride,
                    wide_bytes);
    if (row_stride < (size_t)2 * s->g.block_iq || (row_stride & 1) || (reinterpret_cast<uintptr_t>(rows) & 1))
        return fail(SDR_E_INVALID, "split_block: row_stride %zu < 2*block_iq %d or misaligned", row_stride,
                    2 * s->g.block_iq);
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t hw = (size_t)s->nwide * 8 * s->W;   // dwords of one history parity
    const uint32_t* hin = s->hist + (size_t)s->parity * hw;
    uint32_t* hout = s->hist + (size_t)(s->parity ^ 1) * hw;
    const dim3 grid(cdiv(s->g.block_iq, TT), s->nwide);
    switch (s->W) {
        case 4: hipLaunchKernelGGL(k_split<4>, grid, dim3(64 * SplitK<4>::WAVES), 0, st, wide, wide_stride, hin, hout,
                                   s->bfrag, rows, row_stride, s->clips, s->g.block_iq, s->shift); break;
        case 8: hipLaunchKernelGGL(k_split<8>, grid, dim3(64 * SplitK<8>::WAVES), 0, st, wide, wide_stride, hin, hout,
                                   s->bfrag, rows, row_stride, s->clips, s->g.block_iq, s->shift); break;
        default: hipLaunchKernelGGL(k_split<10>, grid, dim3(64 * SplitK<10>::WAVES), 0, st, wide, wide_stride, hin, hout,
                                    s->bfrag, rows, row_stride, s->clips, s->g.block_iq, s->shift); break;
    }
    LAUNCH_CHECK();
    s->parity ^= 1;
    return SDR_OK;
}

int sdr_split_clips(sdr_split* s, long long* clips, void* stream) {
    if (!s || !clips) return fail(SDR_E_INVALID, "split_clips: null argument");
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = (size_t)s->nwide * (2 * s->W - 1);
    std::vector<unsigned long long> part(n * CLIP_SLOTS);
    if (const int r = copy_records(s->clips, part.data(), part.size(), S(stream))) return r;
    for (size_t i = 0; i < n; i++) {
        unsigned long long sum = 0;
        for (int k = 0; k < CLIP_SLOTS; k++) sum += part[i * CLIP_SLOTS + k];
        clips[i] = (long long)sum;
    }
    return SDR_OK;
}

}  // extern "C"
