// sdr_split16.hip -- the wideband splitter's 16-bit sibling on MI355X (gfx950): one wide int16 I/Q capture at
// W * rf_Fs into the R = 2 W - 1 half-overlapping u8 capture rows at rf_Fs, with a shift per stream and row and a
// peak reading per row (the definition: include/sdr_amd.h, "16-bit wideband splitter"). All integer: every
// output byte, clip count and peak is defined exactly. W, R, T, the taps, the rows, the history rule and the
// sign flip are those of sdr_split.hip, whose header comment describes the GEMM; what differs is the operand.
//
// A sample component x = 256 xh + xl (xh its signed high byte, xl its unsigned low byte) is staged as two int8
// planes in LDS, one byte per component each: xh as it stands, and xl - 128 (the low byte with its top bit
// flipped). Each plane then has exactly the s8 kernel's window geometry: output t's window starts at plane byte
// 2 W (t - t0), 16-, 8- or 4-byte aligned for W = 8, 4, 10. An input dword is one sample (I lo, I hi, Q lo, Q hi)
// and the first window starts on a sample, so the staging needs no byte shift: two samples give one dword of
// each plane by one v_perm each. With the taps e = 128 e_hi + e_lo as in the s8 kernel, four
// v_mfma_i32_16x16x64_i8 accumulators per tile, {xh, xl - 128} x {e_hi, e_lo}, recombine as
//     acc = ((int64)(HH 128 + HL) << 8) + (LH 128 + LL) + 128 S[col],     S[col] = sum of the tap column,
// each 32-bit part below 2^25 in magnitude (128 max_col sum |e| = 2.38e7 at W = 10), while |acc| itself passes
// 2^31 for every W and stays under 2^33.
// Zeros (the history before block 0, the padding past a block's end) go through the same byte transform, so a
// zero sample is (0, -128) in the planes and contributes e (-128) + 128 e = 0.
//
// The epilogue is 64-bit: flip, the lane's row shift (read once per lane), clamp, clip count, max |acc|. The
// peak is reduced like the clip count and kept per row in slotted counters with a 64-bit atomicMax.
//
// History: [2][nwide][T] dwords, the last T samples of the previous block as they came (raw); a block reads
// parity p and writes parity p ^ 1 from its input.
#include "stage_host.h"

#include <vector>

namespace sdrk {
namespace {

#ifndef SPLIT_TT
#define SPLIT_TT 512
#endif
constexpr int TT = SPLIT_TT;   // outputs per workgroup, as k_split
constexpr int SLOTS = 64;      // partial clip and peak counters per row (summed / maxed by the reads)
constexpr int SET_RING = 4;    // pinned staging tables of sdr_split16_set_shifts in flight

bool split16_w(int W) { return W == 4 || W == 8 || W == 10; }

template <int W>
struct Split16K {
    static constexpr int T = 16 * W, K2 = 2 * T, KS = K2 / 64, R = 2 * W - 1;
    static constexpr int NC = (2 * R + 15) / 16;          // column tiles (1, 2, 3)
    static constexpr int TS = NC == 1 ? 4 : 2;            // time groups of waves
    static constexpr int WAVES = NC * TS;
    static constexpr int LDS_BYTES = 2 * W * TT + K2;     // one plane: windows of TT outputs, tails included
    static constexpr int NDW = LDS_BYTES / 4;
    static constexpr int ALIGN = W == 8 ? 16 : W == 4 ? 8 : 4;
    static_assert(K2 % 64 == 0 && NDW % 4 == 0 && TT % (16 * TS) == 0, "tile geometry");
    static_assert(T <= 64 * WAVES, "one thread per history dword");
};
int split16_ncol(int W) { return (2 * (2 * W - 1) + 15) / 16; }

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

// two samples (I lo, I hi, Q lo, Q hi each) -> the high-byte plane's dword and the low-byte plane's (xl - 128)
__device__ __forceinline__ uint32_t plane_hi(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07050301u); }
__device__ __forceinline__ uint32_t plane_lo(uint32_t a, uint32_t b) {
    return __builtin_amdgcn_perm(b, a, 0x06040200u) ^ 0x80808080u;
}

// Grid (ceil(block_iq / TT), nwide). wide: samples as dwords, wide_stride in dwords. bfrag: [2 planes][NC][KS][64
// lanes] v4i; colsum: [16 NC] (0 past 2 R); shifts: [nwide][R]; clips, peaks: [nwide][R][SLOTS].
template <int W>
__global__ __launch_bounds__(64 * Split16K<W>::WAVES) void k_split16(
    const uint32_t* __restrict__ wide, size_t wide_stride, const uint32_t* __restrict__ hist_in,
    uint32_t* __restrict__ hist_out, const v4i* __restrict__ bfrag, const int* __restrict__ colsum,
    const int* __restrict__ shifts, uint8_t* __restrict__ rows, size_t row_stride,
    unsigned long long* __restrict__ clips, unsigned long long* __restrict__ peaks, int block_iq) {
    typedef Split16K<W> G;
    constexpr int T = G::T, KS = G::KS, R = G::R, NC = G::NC, TS = G::TS;
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
    // ---- this wave's tap fragments (constant, L2-resident, lane-major)
    const int ct = wave % NC, ts = wave / NC;
    v4i BH[KS], BL[KS];
#pragma unroll
    for (int kk = 0; kk < KS; kk++) {
        BH[kk] = bfrag[((0 * NC + ct) * KS + kk) * 64 + lane];
        BL[kk] = bfrag[((1 * NC + ct) * KS + kk) * 64 + lane];
    }
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
    // a row's counts and peak of the wave (I and Q lanes, four groups of rows) in one lane, then one atomic each per
    // row and wave into one of SLOTS counters (by workgroup), as k_split does for its clips
    unsigned cnt = nclip + (unsigned)__shfl_xor((int)nclip, 1);
    cnt += (unsigned)__shfl_xor((int)cnt, 16);
    cnt += (unsigned)__shfl_xor((int)cnt, 32);
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

// The tap matrix M of sdr_split_taps(W) as the MFMA's B fragments, laid out as sdr_split.hip lays out its own
// (lane l of fragment (plane, ct, kk) holds M[64 kk + 16 (l >> 4) + j][16 ct + (l & 15)], j < 16, e = 128 hi + lo
// with lo in [-64, 63]), and the column sums S[16 NC].
int split16_fragments(int W, std::vector<int8_t>* f, std::vector<int>* colsum) {
    const int T = 16 * W, R = 2 * W - 1, KS = 2 * T / 64, NC = split16_ncol(W);
    std::vector<int16_t> g((size_t)2 * R * T);
    int total = 0;
    if (const int r = sdr_split_taps(W, g.data(), R * T, &total)) return r;
    f->assign((size_t)2 * NC * KS * 64 * 16, 0);
    colsum->assign((size_t)16 * NC, 0);
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
                    (*f)[((((size_t)0 * NC + ct) * KS + kk) * 64 + l) * 16 + j] = (int8_t)hi;
                    (*f)[((((size_t)1 * NC + ct) * KS + kk) * 64 + l) * 16 + j] = (int8_t)lo;
                    (*colsum)[col] += e;
                }
    return SDR_OK;
}

}  // namespace
}  // namespace sdrk

using namespace sdrk;

struct sdr_split16 {
    int device = 0, mode = 0, W = 0, nwide = 0, block_iq = 0;
    int parity = 0;                          // the history row the next block reads
    uint32_t* hist = nullptr;                // [2][nwide][T]
    v4i* bfrag = nullptr;
    int* colsum = nullptr;                   // [16 NC]
    int* shifts = nullptr;                   // [nwide][R]
    unsigned long long* clips = nullptr;     // [nwide][R][SLOTS]
    unsigned long long* peaks = nullptr;     // [nwide][R][SLOTS]
    // sdr_split16_set_shifts: pinned tables [SET_RING][nwide R] the copies read, and an event behind each copy
    int* stage = nullptr;
    hipEvent_t staged[SET_RING] = {};
    int next = 0;
    size_t rows() const { return (size_t)nwide * (2 * W - 1); }
};

extern "C" {

static int split16_shift_default(int W) { return W == 4 ? 22 : W == 8 ? 23 : 24; }

// the splitter's rule for its arguments; `who` names the caller in the text. *shift <= 0 becomes W's default
static int split16_rule(const char* who, int mode, int W, int nwide, int* shift, int* block_iq) {
    if (mode < 0 || mode > 3) return fail(SDR_E_INVALID, "%s: mode %d not in 0..3", who, mode);
    if (!split16_w(W)) return fail(SDR_E_INVALID, "%s: W %d not 4, 8 or 10", who, W);
    if (nwide < 1 || nwide > 4096) return fail(SDR_E_INVALID, "%s: nwide %d outside [1, 4096]", who, nwide);
    if (*shift <= 0) *shift = split16_shift_default(W);
    if (*shift > 33) return fail(SDR_E_INVALID, "%s: shift %d outside [1, 33]", who, *shift);
    int wide_iq = 0;
    if (const int r = sdr_split_geometry(mode, W, nullptr, nullptr, &wide_iq, nullptr, nullptr)) return r;
    *block_iq = wide_iq / W;
    return SDR_OK;
}

int sdr_split16_shift_for(long long peak, int target, int W) {
    if (!split16_w(W)) return fail(SDR_E_INVALID, "split16_shift_for: W %d not 4, 8 or 10", W);
    if (target < 1 || target > 127) return fail(SDR_E_INVALID, "split16_shift_for: target %d outside [1, 127]", target);
    if (peak < 0) return fail(SDR_E_INVALID, "split16_shift_for: negative peak");
    if (peak == 0) return split16_shift_default(W);
    for (int s = 1; s < 33; s++)
        if (((peak + (1LL << (s - 1))) >> s) <= target) return s;
    return 33;
}

int sdr_split16_check(int mode, int W, int nwide, int shift) {
    int block_iq;
    return split16_rule("split16_check", mode, W, nwide, &shift, &block_iq);
}

int sdr_split16_create(sdr_split16** out, int device, int mode, int W, int nwide, int shift) {
    if (!out) return fail(SDR_E_INVALID, "split16_create: out is NULL");
    *out = nullptr;
    int block_iq = 0;
    if (const int r = split16_rule("split16_create", mode, W, nwide, &shift, &block_iq)) return r;
    std::vector<int8_t> f;
    std::vector<int> cs;
    if (const int r = split16_fragments(W, &f, &cs)) return r;
    sdr_split16* s = nullptr;
    if (const int r = create_begin(&s, device, "split16_create")) return r;
    s->mode = mode;
    s->W = W;
    s->nwide = nwide;
    s->block_iq = block_iq;
    const size_t nr = s->rows(), nh = (size_t)2 * nwide * 16 * W * sizeof(uint32_t);
    const size_t nc = nr * SLOTS * sizeof(unsigned long long);
    const std::vector<int> sh(nr, shift);
    hipError_t e = hipSuccess;
    dev_alloc(e, &s->hist, nh);
    dev_alloc(e, &s->bfrag, f.size());
    dev_alloc(e, &s->colsum, cs.size() * sizeof(int));
    dev_alloc(e, &s->shifts, nr * sizeof(int));
    dev_alloc(e, &s->clips, nc);
    dev_alloc(e, &s->peaks, nc);
    if (e == hipSuccess) e = hipHostMalloc((void**)&s->stage, SET_RING * nr * sizeof(int), hipHostMallocDefault);
    for (int k = 0; k < SET_RING; k++)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->staged[k], hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemcpy(s->bfrag, f.data(), f.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->colsum, cs.data(), cs.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->shifts, sh.data(), nr * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(s->hist, 0, nh);
    if (e == hipSuccess) e = hipMemset(s->clips, 0, nc);
    if (e == hipSuccess) e = hipMemset(s->peaks, 0, nc);
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
    const size_t nc = s->rows() * SLOTS * sizeof(unsigned long long);
    HIP_TRY(hipMemsetAsync(s->hist, 0, (size_t)2 * s->nwide * 16 * s->W * sizeof(uint32_t), S(stream)));
    HIP_TRY(hipMemsetAsync(s->clips, 0, nc, S(stream)));
    HIP_TRY(hipMemsetAsync(s->peaks, 0, nc, S(stream)));
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
    const size_t wide_bytes = (size_t)4 * s->W * s->block_iq;
    if (wide_stride < wide_bytes || (wide_stride & 3) || (reinterpret_cast<uintptr_t>(wide) & 3))
        return fail(SDR_E_INVALID, "split16_block: wide_stride %zu < 4*W*block_iq %zu, or not 4-byte aligned", wide_stride,
                    wide_bytes);
    if (row_stride < (size_t)2 * s->block_iq || (row_stride & 1) || (reinterpret_cast<uintptr_t>(rows) & 1))
        return fail(SDR_E_INVALID, "split16_block: row_stride %zu < 2*block_iq %d or misaligned", row_stride,
                    2 * s->block_iq);
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t hw = (size_t)s->nwide * 16 * s->W;   // dwords of one history parity
    const uint32_t* hin = s->hist + (size_t)s->parity * hw;
    uint32_t* hout = s->hist + (size_t)(s->parity ^ 1) * hw;
    const uint32_t* in = reinterpret_cast<const uint32_t*>(wide);
    const dim3 grid(cdiv(s->block_iq, TT), s->nwide);
    switch (s->W) {
        case 4: hipLaunchKernelGGL(k_split16<4>, grid, dim3(64 * Split16K<4>::WAVES), 0, st, in, wide_stride / 4, hin, hout,
                                   s->bfrag, s->colsum, s->shifts, rows, row_stride, s->clips, s->peaks, s->block_iq); break;
        case 8: hipLaunchKernelGGL(k_split16<8>, grid, dim3(64 * Split16K<8>::WAVES), 0, st, in, wide_stride / 4, hin, hout,
                                   s->bfrag, s->colsum, s->shifts, rows, row_stride, s->clips, s->peaks, s->block_iq); break;
        default: hipLaunchKernelGGL(k_split16<10>, grid, dim3(64 * Split16K<10>::WAVES), 0, st, in, wide_stride / 4, hin,
                                    hout, s->bfrag, s->colsum, s->shifts, rows, row_stride, s->clips, s->peaks,
                                    s->block_iq); break;
    }
    LAUNCH_CHECK();
    s->parity ^= 1;
    return SDR_OK;
}

int sdr_split16_clips(sdr_split16* s, long long* clips, void* stream) {
    if (!s || !clips) return fail(SDR_E_INVALID, "split16_clips: null argument");
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = s->rows();
    std::vector<unsigned long long> part(n * SLOTS);
    if (const int r = copy_records(s->clips, part.data(), part.size(), S(stream))) return r;
    for (size_t i = 0; i < n; i++) {
        unsigned long long sum = 0;
        for (int k = 0; k < SLOTS; k++) sum += part[i * SLOTS + k];
        clips[i] = (long long)sum;
    }
    return SDR_OK;
}

int sdr_split16_peaks(sdr_split16* s, long long* peaks, int clear, void* stream) {
    if (!s || !peaks) return fail(SDR_E_INVALID, "split16_peaks: null argument");
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = s->rows();
    std::vector<unsigned long long> part(n * SLOTS);
    // the clearing read's memset follows the copy on the stream, and both are waited for
    HIP_TRY(hipMemcpyAsync(part.data(), s->peaks, part.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           S(stream)));
    if (clear) HIP_TRY(hipMemsetAsync(s->peaks, 0, part.size() * sizeof(unsigned long long), S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));
    for (size_t i = 0; i < n; i++) {
        unsigned long long mx = 0;
        for (int k = 0; k < SLOTS; k++) mx = part[i * SLOTS + k] > mx ? part[i * SLOTS + k] : mx;
        peaks[i] = (long long)mx;
    }
    return SDR_OK;
}

}  // extern "C"
