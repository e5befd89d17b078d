// sdr_scan.hip -- band scan of the shared-capture rows on MI355X (gfx950): a batched power spectrum
// whose bins are the tuner's 1 kHz steps (the reference's estimatePSD, src/fourier.cpp:
// non-overlapping segments, Hann window, |X|^2 per bin, average over segments), and the host-side
// picker that turns a spectrum into the tuner's "src khz" list.
//
// Per block and row: S_b = block_iq / N segments of N = rf_Fs / 1000 samples from the block's first
// sample on. Per segment x[n] = (u8 - 128) / 128, times the f32 Hann table, then
//     X[k] = sum_n xw[n] e^(-j 2 pi k n / N),  p[k] = re^2 + im^2
// as a two-pass mixed-radix DFT in LDS, N = N1 x N2 (48 x 50, 36 x 40, 32 x 36), n = N2 n1 + n2,
// k = k1 + N1 k2:
//   pass 1   Y[k1][n2] = (sum_n1 xw[N2 n1 + n2] W_N1^(n1 k1)) W_N^(n2 k1)   N2 direct N1-point DFTs
//   pass 2   X[k1 + N1 k2] = sum_n2 Y[k1][n2] W_N2^(n2 k2)                 N1 direct N2-point DFTs
// Every twiddle is an entry of the tuner's correctly rounded rotator table (sdr_tuner_table; index
// arithmetic mod N, W_N1 = T[N2 m], W_N2 = T[N1 m], laid out by the host as the two passes' DFT
// matrices); no sincosf. A wave owns a block of output indices (k1 in pass 1, k2 in pass 2) and its
// lanes the independent transforms (n2, then k1), so the DFT-matrix twiddles are the same for all
// lanes: a matrix row's block comes through the scalar cache into SGPRs in wide scalar loads, and
// each complex multiply-add is four v_fma_f32. LDS holds one plane of N (padded) complex f32;
// both passes work in place (all reads, barrier, all writes). Pass 1 stores Y transposed with an odd
// row pitch, so that its 8-byte stores spread over the banks and pass 2 reads consecutive addresses.
//
// Fixed summation order (a row's result is bit-identical from run to run and whatever rows share the
// batch): a workgroup adds the p[k] of SEG_PER_WG consecutive segments in registers, in order, and
// stores the partial; k_scan_accum then adds a block's partials in order and the sum to A.
#include "stage_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace sdrk {
namespace {

constexpr int SCAN_WAVES = 4;
constexpr int SCAN_THREADS = 64 * SCAN_WAVES;
// A/B builds only (-DSCAN_SEG_PER_WG=n, -DSCAN_UNROLL=n; profiles/r08/scan/README.md)
#ifndef SCAN_SEG_PER_WG
#define SCAN_SEG_PER_WG 3
#endif
#ifndef SCAN_UNROLL
#define SCAN_UNROLL 2
#endif
constexpr int SEG_PER_WG = SCAN_SEG_PER_WG;   // segments a workgroup sums (S_b = 30, 36, 33, 33: all multiples of 3)

struct ScanGeom {
    int N, N1, N2, block_iq;
};
bool scan_geom(int mode, ScanGeom* g) {
    switch (mode) {
        case 0: *g = {2400, 48, 50, 73500}; return true;
        case 1: *g = {1440, 36, 40, 52920}; return true;
        case 2: *g = {2400, 48, 50, 80000}; return true;
        case 3: *g = {1152, 32, 36, 38400}; return true;
        default: return false;
    }
}

// acc[r] = sum_n in[n * pitch] W_F^(n (k0 + r)), r < R. W is the pass's DFT matrix [F][F] (entry [n][k]
// = W_F^(n k) = (c, s), taken as c - j s) from column k0 on; k0 is wave-uniform, so a row's R twiddles
// are consecutive scalar loads. `in` already points at the lane's transform. (A block's tail past F
// reads on into the next row -- the matrix is padded by one block -- and is dropped by the caller.)
template <int F, int R>
__device__ __forceinline__ void dft_block(const float2* in, int pitch, const float2* __restrict__ W,
                                          float (&re)[R], float (&im)[R]) {
#pragma unroll
    for (int r = 0; r < R; r++) {
        re[r] = 0.0f;
        im[r] = 0.0f;
    }
#pragma unroll SCAN_UNROLL
    for (int n = 0; n < F; n++) {
        const float2 x = in[n * pitch];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float2 w = W[n * F + r];
            re[r] = fmaf(x.x, w.x, re[r]);
            re[r] = fmaf(x.y, w.y, re[r]);
            im[r] = fmaf(x.y, w.x, im[r]);
            im[r] = fmaf(-x.x, w.y, im[r]);
        }
    }
}

// Grid (S_b / SEG_PER_WG, nsrc). part: [nsrc][gridDim.x][N]. T: the rotator table [N]; W1 [N1][N1] and
// W2 [N2][N2]: the passes' DFT matrices, W1[n][k] = T[N2 ((n k) mod N1)], W2[n][k] = T[N1 ((n k) mod N2)].
template <int N1, int N2>
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_psd(const uint8_t* __restrict__ iq, size_t iq_stride,
                                                           const float* __restrict__ win,
                                                           const float2* __restrict__ T,
                                                           const float2* __restrict__ W1,
                                                           const float2* __restrict__ W2,
                                                           float* __restrict__ part) {
    constexpr int N = N1 * N2;
    constexpr int P = N1 | 1;                            // odd pitch of the transposed Y rows
    constexpr int R1 = (N1 + SCAN_WAVES - 1) / SCAN_WAVES, R2 = (N2 + SCAN_WAVES - 1) / SCAN_WAVES;
    constexpr int PLANE = N2 * P > N ? N2 * P : N;
    static_assert(N1 <= 64 && N2 <= 64 && N % 8 == 0, "one lane per transform; 16-byte loads");
    static_assert(SCAN_WAVES * R1 - N1 <= 16 && SCAN_WAVES * R2 - N2 <= 16, "the DFT matrices' padding");
    __shared__ __attribute__((aligned(16))) float2 plane[PLANE];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int row = blockIdx.y, chunk = blockIdx.x;
    const uint8_t* src = iq + (size_t)row * iq_stride + (size_t)chunk * SEG_PER_WG * 2 * N;
    const bool wide = (reinterpret_cast<uintptr_t>(src) & 15) == 0;   // (2 N is a multiple of 16)
    const int l1 = min(lane, N2 - 1), l2 = min(lane, N1 - 1);         // idle lanes read a valid transform
    const int k10 = wave * R1, k20 = wave * R2;
    float pw[R2];
#pragma unroll
    for (int r = 0; r < R2; r++) pw[r] = 0.0f;

    for (int seg = 0; seg < SEG_PER_WG; seg++, src += 2 * N) {
        // ---- u8 pairs -> (u8 - 128) / 128, times the window, into the plane in natural order
        if (wide) {
            for (int i = t; i < N / 8; i += SCAN_THREADS) {
                const uint4 v = reinterpret_cast<const uint4*>(src)[i];
                const float4 wa = reinterpret_cast<const float4*>(win)[2 * i];
                const float4 wb = reinterpret_cast<const float4*>(win)[2 * i + 1];
                const uint32_t u[4] = {v.x, v.y, v.z, v.w};
                const float w[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const uint32_t h = u[j >> 1] >> (16 * (j & 1));
                    const float xi = ((float)(int)(h & 255u) - 128.0f) * 0.0078125f;
                    const float xq = ((float)(int)((h >> 8) & 255u) - 128.0f) * 0.0078125f;
                    plane[8 * i + j] = make_float2(xi * w[j], xq * w[j]);
                }
            }
        } else {   // a row that is only 2-byte aligned (the C ABI asks no more)
            for (int i = t; i < N; i += SCAN_THREADS) {
                const uint32_t h = reinterpret_cast<const uint16_t*>(src)[i];
                const float xi = ((float)(int)(h & 255u) - 128.0f) * 0.0078125f;
                const float xq = ((float)(int)((h >> 8) & 255u) - 128.0f) * 0.0078125f;
                const float w = win[i];
                plane[i] = make_float2(xi * w, xq * w);
            }
        }
        __syncthreads();
        // ---- pass 1: lane = n2, wave = block of k1
        {
            float re[R1], im[R1];
            dft_block<N1, R1>(plane + l1, N2, W1 + k10, re, im);
            __syncthreads();   // every wave has read the natural-order plane
            if (lane < N2) {
#pragma unroll
                for (int r = 0; r < R1; r++) {
                    const int k1 = k10 + r;
                    if (k1 < N1) {
                        const float2 w = T[(lane * k1) % N];
                        const float yr = fmaf(re[r], w.x, im[r] * w.y);
                        const float yi = fmaf(im[r], w.x, -(re[r] * w.y));
                        plane[lane * P + k1] = make_float2(yr, yi);
                    }
                }
            }
        }
        __syncthreads();
        // ---- pass 2: lane = k1, wave = block of k2
        {
            float re[R2], im[R2];
            dft_block<N2, R2>(plane + l2, P, W2 + k20, re, im);
#pragma unroll
            for (int r = 0; r < R2; r++) pw[r] += fmaf(re[r], re[r], im[r] * im[r]);
        }
        __syncthreads();   // the plane is free for the next segment
    }
    if (lane < N1) {
        float* out = part + ((size_t)row * gridDim.x + chunk) * N;
#pragma unroll
        for (int r = 0; r < R2; r++) {
            const int k2 = k20 + r;
            if (k2 < N2) out[lane + N1 * k2] = pw[r];
        }
    }
}

// A[row][k] += part[row][0][k] + part[row][1][k] + ... (in this order)
__global__ __launch_bounds__(BLK) void k_scan_accum(float* __restrict__ A, const float* __restrict__ part, int N,
                                                    int chunks, int total) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= total) return;
    const int row = i / N, k = i - row * N;
    const float* p = part + (size_t)row * chunks * N + k;
    float s = p[0];
    for (int c = 1; c < chunks; c++) s += p[(size_t)c * N];
    A[i] += s;
}

// RN32(0.5 - 0.5 cos(2 pi j / N)), evaluated in f64 (the reference's sin^2(pi j / N))
void scan_window(int N, float* w) {
    const double two_pi = 2.0 * 3.14159265358979323846;
    for (int j = 0; j < N; j++) w[j] = (float)(0.5 - 0.5 * std::cos(two_pi * (double)j / (double)N));
}

}  // namespace
}  // namespace sdrk

using namespace sdrk;

struct sdr_scan {
    int device = 0, mode = 0, nsrc = 0;
    ScanGeom g{};
    int seg_block = 0, chunks = 0;
    long long segments = 0;            // accumulated per row since the last reset
    float2* T = nullptr;               // rotator table [N], then the DFT matrices W1, W2 (k_scan_psd)
    size_t w1_off = 0, w2_off = 0;     // their offsets in T, in entries
    float *win = nullptr, *part = nullptr, *A = nullptr;
};

extern "C" {

int sdr_scan_geometry(int mode, int* n_bins, int* segments_per_block, int* block_iq) {
    ScanGeom g;
    if (!scan_geom(mode, &g)) return fail(SDR_E_INVALID, "scan_geometry: mode %d not in 0..3", mode);
    if (n_bins) *n_bins = g.N;
    if (segments_per_block) *segments_per_block = g.block_iq / g.N;
    if (block_iq) *block_iq = g.block_iq;
    return SDR_OK;
}

int sdr_scan_window(int mode, float* w, int max, int* n) {
    ScanGeom g;
    if (!scan_geom(mode, &g) || !n) return fail(SDR_E_INVALID, "scan_window: bad mode or null n");
    if (w && max < g.N) return fail(SDR_E_INVALID, "scan_window: room for %d of %d entries", max, g.N);
    *n = g.N;
    if (w) scan_window(g.N, w);
    return SDR_OK;
}

void sdr_scan_opts_default(sdr_scan_opts* o) {
    if (!o) return;
    o->half_width_khz = 100;
    o->step_khz = 100;
    o->first_khz = 0;
    o->sep_khz = 150;
    o->guard_khz = 100;
    o->thr_db = 10.0f;
}

int sdr_scan_pick(int mode, const float* psd_row, const sdr_scan_opts* o, int32_t* khz, float* db, int max, int* n) {
    ScanGeom g;
    if (!scan_geom(mode, &g)) return fail(SDR_E_INVALID, "scan_pick: mode %d not in 0..3", mode);
    if (!psd_row || !o || !n || max < 0 || (max > 0 && (!khz || !db)))
        return fail(SDR_E_INVALID, "scan_pick: null argument");
    const int N = g.N, W = o->half_width_khz;
    if (W < 0 || 2 * W >= N || o->step_khz < 1 || o->sep_khz < 0 || o->guard_khz < 0 || 2 * o->guard_khz > N ||
        !std::isfinite(o->thr_db))
        return fail(SDR_E_INVALID, "scan_pick: options outside 0 <= half_width < N/2, step >= 1, sep >= 0, "
                                   "0 <= guard <= N/2, finite thr_db");
    // channel power: the 2 W + 1 bins around k, added in ascending d
    std::vector<double> C(N, 0.0);
    for (int d = -W; d <= W; d++)
        for (int k = 0; k < N; k++) C[k] += (double)psd_row[((k + d) % N + N) % N];
    std::vector<double> sorted(C);
    std::nth_element(sorted.begin(), sorted.begin() + (N - 1) / 2, sorted.end());
    const double F = sorted[(N - 1) / 2];
    const double need = F * std::pow(10.0, (double)o->thr_db / 10.0);
    struct Cand {
        int khz;
        double c;
    };
    std::vector<Cand> cand;
    const long long step = o->step_khz;
    for (int f = -N / 2 + o->guard_khz; f <= N / 2 - o->guard_khz; f++)
        if ((((long long)f - o->first_khz) % step + step) % step == 0) cand.push_back({f, C[(f % N + N) % N]});
    std::vector<Cand> found;
    for (size_t i = 0; i < cand.size(); i++) {
        const Cand& a = cand[i];
        if (!(a.c > 0.0) || !(a.c >= need)) continue;
        bool top = true;   // (candidates are in ascending khz: the neighbours within sep are contiguous)
        for (size_t j = i; top && j-- > 0 && a.khz - cand[j].khz <= o->sep_khz;) top = cand[j].c < a.c;
        for (size_t j = i + 1; top && j < cand.size() && cand[j].khz - a.khz <= o->sep_khz; j++) top = cand[j].c <= a.c;
        if (top) found.push_back(a);
    }
    std::stable_sort(found.begin(), found.end(), [](const Cand& a, const Cand& b) { return a.c > b.c; });
    *n = (int)found.size();
    for (int i = 0; i < max && i < (int)found.size(); i++) {
        khz[i] = found[i].khz;
        db[i] = F > 0.0 ? (float)(10.0 * std::log10(found[i].c / F)) : HUGE_VALF;
    }
    return SDR_OK;
}

int sdr_scan_create(sdr_scan** out, int device, int mode, int nsrc) {
    if (!out) return fail(SDR_E_INVALID, "scan_create: out is NULL");
    *out = nullptr;
    ScanGeom g;
    if (!scan_geom(mode, &g)) return fail(SDR_E_INVALID, "scan_create: mode %d not in 0..3", mode);
    if (nsrc < 1 || nsrc > 65535) return fail(SDR_E_INVALID, "scan_create: nsrc %d outside [1, 65535]", nsrc);
    sdr_scan* s = nullptr;
    if (const int r = create_begin(&s, device, "scan_create")) return r;
    s->mode = mode;
    s->nsrc = nsrc;
    s->g = g;
    s->seg_block = g.block_iq / g.N;
    s->chunks = s->seg_block / SEG_PER_WG;
    if (s->chunks * SEG_PER_WG != s->seg_block) {
        delete s;
        return fail(SDR_E_INVALID, "scan_create: %d segments per block are no multiple of %d", g.block_iq / g.N, SEG_PER_WG);
    }
    std::vector<float> tab((size_t)2 * g.N), win(g.N);
    int n = 0;
    const int rt = sdr_tuner_table(mode, tab.data(), g.N, &n);
    if (rt != SDR_OK || n != g.N) {
        delete s;
        return fail(SDR_E_INVALID, "scan_create: no rotator table of %d entries for mode %d", g.N, mode);
    }
    // the passes' DFT matrices behind the table, each padded by a block of entries (dft_block)
    s->w1_off = g.N;
    s->w2_off = s->w1_off + (size_t)g.N1 * g.N1 + 16;
    tab.resize(2 * (s->w2_off + (size_t)g.N2 * g.N2 + 16), 0.0f);
    for (int pass = 0; pass < 2; pass++) {
        const int F = pass ? g.N2 : g.N1, step = pass ? g.N1 : g.N2;
        float* W = tab.data() + 2 * (pass ? s->w2_off : s->w1_off);
        for (int nn = 0; nn < F; nn++)
            for (int k = 0; k < F; k++) {
                const int i = step * ((nn * k) % F);
                W[2 * (nn * F + k)] = tab[2 * i];
                W[2 * (nn * F + k) + 1] = tab[2 * i + 1];
            }
    }
    scan_window(g.N, win.data());
    const size_t nA = (size_t)nsrc * g.N;
    hipError_t e = hipSuccess;
    dev_alloc(e, &s->T, tab.size() * sizeof(float));
    dev_alloc(e, &s->win, win.size() * sizeof(float));
    dev_alloc(e, &s->part, nA * s->chunks * sizeof(float));
    dev_alloc(e, &s->A, nA * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(s->T, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->win, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(s->A, 0, nA * sizeof(float));
    return create_done(e, s, out, sdr_scan_destroy, "scan_create");
}

int sdr_scan_destroy(sdr_scan* s) {
    if (!s) return fail(SDR_E_INVALID, "scan_destroy: null scanner");
    return destroy_handle(s, {s->T, s->win, s->part, s->A});
}

int sdr_scan_reset(sdr_scan* s, void* stream) {
    if (!s) return fail(SDR_E_INVALID, "scan_reset: null scanner");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemsetAsync(s->A, 0, (size_t)s->nsrc * s->g.N * sizeof(float), (hipStream_t)stream));
    s->segments = 0;
    return SDR_OK;
}

int sdr_scan_block(sdr_scan* s, const uint8_t* iq, size_t iq_stride, void* stream) {
    if (!s || !iq) return fail(SDR_E_INVALID, "scan_block: null argument");
    if (iq_stride < (size_t)2 * s->g.block_iq || (iq_stride & 1) || (reinterpret_cast<uintptr_t>(iq) & 1))
        return fail(SDR_E_INVALID, "scan_block: iq_stride %zu < 2*block_iq %d or misaligned", iq_stride,
                    2 * s->g.block_iq);
    HIP_TRY(hipSetDevice(s->device));
    const dim3 grid(s->chunks, s->nsrc), blk(SCAN_THREADS);
    hipStream_t st = (hipStream_t)stream;
    switch (s->g.N) {
        case 2400: hipLaunchKernelGGL((k_scan_psd<48, 50>), grid, blk, 0, st, iq, iq_stride, s->win, s->T, s->T + s->w1_off,
                                      s->T + s->w2_off, s->part); break;
        case 1440: hipLaunchKernelGGL((k_scan_psd<36, 40>), grid, blk, 0, st, iq, iq_stride, s->win, s->T, s->T + s->w1_off,
                                      s->T + s->w2_off, s->part); break;
        default: hipLaunchKernelGGL((k_scan_psd<32, 36>), grid, blk, 0, st, iq, iq_stride, s->win, s->T, s->T + s->w1_off,
                                      s->T + s->w2_off, s->part); break;
    }
    LAUNCH_CHECK();
    const int total = s->nsrc * s->g.N;
    hipLaunchKernelGGL(k_scan_accum, dim3(cdiv(total, BLK)), dim3(BLK), 0, st, s->A, s->part, s->g.N, s->chunks, total);
    LAUNCH_CHECK();
    s->segments += s->seg_block;
    return SDR_OK;
}

int sdr_scan_psd(sdr_scan* s, float* psd, long long* segments, void* stream) {
    if (!s || !psd) return fail(SDR_E_INVALID, "scan_psd: null argument");
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = (size_t)s->nsrc * s->g.N;
    if (const int r = copy_records(s->A, psd, n, S(stream))) return r;
    if (s->segments > 0) {
        const float S = (float)s->segments;
        for (size_t i = 0; i < n; i++) psd[i] = psd[i] / S;
    }
    if (segments) *segments = s->segments;
    return SDR_OK;
}

}  // extern "C"
