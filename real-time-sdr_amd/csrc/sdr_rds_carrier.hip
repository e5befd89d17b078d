// sdr_rds_carrier.hip -- RDS carrier-phase derotator on MI355X (gfx950): the in-phase and quadrature rows of
// the RDS chain are turned onto one axis by the phase of their squared signal, estimated window by window of
// the stream. No reference counterpart; the definition is in include/sdr_amd.h (sdr_rds_carrier_*) and
// tests/rds_carrier_model.py reproduces every bit. One quantisation, then all integer.
//
// k_rds_carrier, one wave per channel (grid nch, 64 threads), as k_rds_track is laid out:
//   stage     both rows go to LDS quantised, a sample's pair packed into one word, the loads of a round all in
//             flight (16-byte loads where both rows are aligned); a non-finite sample ends the call before any
//             state is touched
//   walk      the chunk is cut where the stream's windows end. Within a piece (c, s) is constant: lane l takes
//             the samples l, l + 64, ... of it, writes y over the pair and adds to its three int64 sums; a
//             butterfly gives the piece's sums to every lane. Where a window ends, the smoothing, the two
//             CORDICs and the new (c, s) are wave-uniform: every lane computes them.
//   store     y * 2^-qshift goes out, with 16-byte stores where the output row is aligned
// A call longer than CAR_CHUNK samples runs as consecutive chunks through the same LDS: the definition does
// not depend on how the stream is cut, so that is the same result.
// The state is one 128-byte record per channel in HBM, read by every lane and written back by lane 0 with
// plain vector stores.
#include "stage_host.h"

#include <cstring>

struct sdr_rds_carrier {
    int device = 0, nch = 0, mode = 0;
    sdr_rds_carrier_opts opts{};
    void* st = nullptr;                     // [nch] CarState (device)
    sdr_rds_carrier_stats* stats = nullptr; // [nch] (device), gathered by k_carrier_stats
};

namespace sdrk {
namespace {

constexpr int CAR_W = SDR_RDS_CARRIER_W;
constexpr int CAR_N = SDR_RDS_CARRIER_CORDIC_N;
constexpr int CAR_CHUNK = 3072;                    // samples staged at once: a block (2836) in one round of loads
constexpr int CAR_ONE = 1 << 14;
constexpr int CAR_X0 = 326016437;                  // 2^29 / prod sqrt(1 + 4^-i), i < 24
static_assert(CAR_CHUNK % 4 == 0, "a chunk starts on a 16-byte boundary of an aligned row");
static_assert((long long)CAR_W << 31 == 1ll << 42, "a window's sums are at most 2^42");
static_assert(32767ll * 23173 + (1 << 13) < (1ll << 31), "the rotation fits int32");

struct CarHead {                                   // the wave-uniform state, 72 bytes
    int64_t pr, pi, pt;            // the current window's sums so far
    int64_t sr, si, st;            // the smoothed sums
    int32_t phi, c, s;             // the phase in use and its Q14 vector
    int32_t wcnt;                  // samples of the current window so far (< W)
    uint32_t windows, resets;
};
struct alignas(64) CarState {                      // 128 bytes
    CarHead h;
};
static_assert(sizeof(CarState) == 128, "CarState is two 64-byte lines");

__device__ __forceinline__ int quant(float x, int scale_bits) {
    // rint(clamp(x * 2^k, +-32767)): the clamp first, so that an overflowing product is clamped too
    const float y = fminf(fmaxf(x * __int_as_float(scale_bits), -32767.0f), 32767.0f);
    return __float2int_rn(y);
}
__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ int pack(int qi, int qq) { return (qi & 0xFFFF) | (int)((unsigned)qq << 16); }

__device__ __forceinline__ void first_window(CarHead& s) {    // the stream starts again; the counters stay
    s.pr = s.pi = s.pt = 0;
    s.sr = s.si = s.st = 0;
    s.phi = 0, s.c = CAR_ONE, s.s = 0;
    s.wcnt = 0;
}

__device__ __forceinline__ constexpr int car_atan(int i) {
    constexpr int A[CAR_N] = {536870912, 316933406, 167458907, 85004756, 42667331, 21354465, 10679838, 5340245,
                              2670163,   1335087,   667544,    333772,   166886,   83443,    41722,    20861,
                              10430,     5215,      2608,      1304,     652,      326,      163,      81};
    return A[i];
}

// the end of a window: smooth, take the angle, halve it on the branch nearer the last, make the next (c, s)
__device__ void window_end(CarHead& s, int k) {
    s.sr += (s.pr - s.sr) >> k;
    s.si += (s.pi - s.si) >> k;
    s.st += (s.pt - s.st) >> k;
    s.pr = s.pi = s.pt = 0;
    s.wcnt = 0;
    s.windows++;
    const long long ar = s.sr < 0 ? -s.sr : s.sr, ai = s.si < 0 ? -s.si : s.si, m = ar > ai ? ar : ai;
    if (m == 0) return;
    const int bl = 64 - __clzll(m);
    int x, y;
    if (bl > 29) x = (int)(s.sr >> (bl - 29)), y = (int)(s.si >> (bl - 29));
    else x = (int)(s.sr * (1ll << (29 - bl))), y = (int)(s.si * (1ll << (29 - bl)));
    uint32_t z = 0;
    if (x < 0) x = -x, y = -y, z = 0x80000000u;
#pragma unroll
    for (int i = 0; i < CAR_N; i++) {
        const int xs = x >> i, ys = y >> i;
        if (y >= 0) x += ys, y -= xs, z += (uint32_t)car_atan(i);
        else x -= ys, y += xs, z -= (uint32_t)car_atan(i);
    }
    int phi = (int)z >> 1;
    const int d = (int)((uint32_t)phi - (uint32_t)s.phi);
    if (d > (1 << 30) || d < -(1 << 30)) phi = (int)((uint32_t)phi + 0x80000000u);
    s.phi = phi;
    int zr = phi;
    const bool neg = zr > (1 << 30) || zr < -(1 << 30);
    if (neg) zr = (int)((uint32_t)zr - 0x80000000u);
    x = CAR_X0, y = 0;
#pragma unroll
    for (int i = 0; i < CAR_N; i++) {
        const int xs = x >> i, ys = y >> i;
        if (zr >= 0) x -= ys, y += xs, zr -= car_atan(i);
        else x += ys, y -= xs, zr += car_atan(i);
    }
    const int c = (x + (1 << 14)) >> 15, sn = (y + (1 << 14)) >> 15;
    s.c = neg ? -c : c, s.s = neg ? -sn : sn;
}

__global__ __launch_bounds__(64) void k_rds_carrier(CarState* __restrict__ st_all, const float* __restrict__ xi,
                                                    size_t stride_i, const float* __restrict__ xq, size_t stride_q,
                                                    int n, float* __restrict__ out, size_t out_stride, int scale_bits,
                                                    int inv_scale_bits, int k) {
    __shared__ __attribute__((aligned(16))) int Q[CAR_CHUNK];
    const int ch = blockIdx.x, lane = threadIdx.x;
    if (n <= 0) return;
    CarState* sp = st_all + ch;
    const float* ic = xi + (size_t)ch * stride_i;
    const float* qc = xq + (size_t)ch * stride_q;
    float* oc = out + (size_t)ch * out_stride;
    CarHead s = sp->h;             // wave-uniform
    const bool vec_in = ((reinterpret_cast<uintptr_t>(ic) | reinterpret_cast<uintptr_t>(qc)) & 15) == 0;
    const bool vec_out = (reinterpret_cast<uintptr_t>(oc) & 15) == 0;
    const float inv_scale = __int_as_float(inv_scale_bits);
    // ---- a call of more than one chunk: look for a non-finite sample before any of it is used
    bool bad = false;
    if (n > CAR_CHUNK) {
        for (int i = lane; i < n; i += 64) bad |= !(finite_bits(ic[i]) && finite_bits(qc[i]));
        bad = __any(bad);
    }
    for (int c0 = 0; c0 < n && !bad; c0 += CAR_CHUNK) {
        const int m = min(CAR_CHUNK, n - c0);
        const float* ir = ic + c0;                 // c0 is a multiple of 4: the alignment of the rows holds
        const float* qr = qc + c0;
        // ---- stage and quantise: every load of a round in flight, then the LDS writes
        int i_tail = 0;
        if (vec_in) {
            constexpr int U4 = 6;
            const int n4 = m >> 2;
            for (int q0 = lane; q0 < n4; q0 += 64 * U4) {
                // unconditional at a clamped index (lanes past the row rewrite its last vector)
                float4 vi[U4], vq[U4];
#pragma unroll
                for (int u = 0; u < U4; u++) {
                    vi[u] = reinterpret_cast<const float4*>(ir)[min(q0 + 64 * u, n4 - 1)];
                    vq[u] = reinterpret_cast<const float4*>(qr)[min(q0 + 64 * u, n4 - 1)];
                }
#pragma unroll
                for (int u = 0; u < U4; u++) {
                    const int j = 4 * min(q0 + 64 * u, n4 - 1);
                    bad |= !(finite_bits(vi[u].x) && finite_bits(vi[u].y) && finite_bits(vi[u].z) && finite_bits(vi[u].w));
                    bad |= !(finite_bits(vq[u].x) && finite_bits(vq[u].y) && finite_bits(vq[u].z) && finite_bits(vq[u].w));
                    Q[j] = pack(quant(vi[u].x, scale_bits), quant(vq[u].x, scale_bits));
                    Q[j + 1] = pack(quant(vi[u].y, scale_bits), quant(vq[u].y, scale_bits));
                    Q[j + 2] = pack(quant(vi[u].z, scale_bits), quant(vq[u].z, scale_bits));
                    Q[j + 3] = pack(quant(vi[u].w, scale_bits), quant(vq[u].w, scale_bits));
                }
            }
            i_tail = n4 * 4;
        }
        constexpr int U = 6;
        for (int i0 = i_tail + lane; i0 < m; i0 += 64 * U) {
            float vi[U], vq[U];
#pragma unroll
            for (int u = 0; u < U; u++) vi[u] = ir[min(i0 + 64 * u, m - 1)], vq[u] = qr[min(i0 + 64 * u, m - 1)];
#pragma unroll
            for (int u = 0; u < U; u++) {
                bad |= !(finite_bits(vi[u]) && finite_bits(vq[u]));
                Q[min(i0 + 64 * u, m - 1)] = pack(quant(vi[u], scale_bits), quant(vq[u], scale_bits));
            }
        }
        bad = __any(bad);
        if (bad) break;
        __syncthreads();
        // ---- walk: pieces that end where a window of the stream or the chunk ends
        for (int a = 0; a < m;) {
            const int b = min(m, a + CAR_W - s.wcnt);
            long long pr = 0, pi = 0, pt = 0;
            for (int i = a + lane; i < b; i += 64) {
                const int w = Q[i];
                const int qi = (int)(short)(w & 0xFFFF), qq = w >> 16;
                const int y = (qi * s.c + qq * s.s + (1 << 13)) >> 14;
                Q[i] = min(max(y, -32767), 32767);
                const int ii = qi * qi, q2 = qq * qq;
                pr += ii - q2, pi += 2 * qi * qq, pt += ii + q2;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) pr += __shfl_xor(pr, o), pi += __shfl_xor(pi, o), pt += __shfl_xor(pt, o);
            s.pr += pr, s.pi += pi, s.pt += pt;
            s.wcnt += b - a;
            if (s.wcnt == CAR_W) window_end(s, k);
            a = b;
        }
        __syncthreads();
        // ---- store: y * 2^-qshift, exact
        float* orow = oc + c0;
        int o_tail = 0;
        if (vec_out) {
            const int n4 = m >> 2;
            for (int j = lane; j < n4; j += 64) {
                const int4 v = reinterpret_cast<const int4*>(Q)[j];
                reinterpret_cast<float4*>(orow)[j] =
                    make_float4((float)v.x * inv_scale, (float)v.y * inv_scale, (float)v.z * inv_scale, (float)v.w * inv_scale);
            }
            o_tail = n4 * 4;
        }
        for (int i = o_tail + lane; i < m; i += 64) orow[i] = (float)Q[i] * inv_scale;
        __syncthreads();           // the next chunk's staging overwrites Q
    }
    if (bad) {                     // uniform: nothing of the call was used, the stream starts again
        const float nan = __int_as_float(0x7FC00000);
        for (int i = lane; i < n; i += 64) oc[i] = nan;
        first_window(s);
        s.resets++;
    }
    if (lane == 0) sp->h = s;
}

__global__ void k_carrier_reset(CarState* st, int nch) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= nch) return;
    CarHead s{};
    first_window(s);
    st[ch].h = s;
}

__global__ void k_carrier_stats(const CarState* st, sdr_rds_carrier_stats* out, int nch) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= nch) return;
    const CarHead& s = st[ch].h;
    sdr_rds_carrier_stats r;
    r.sr = s.sr, r.si = s.si, r.st = s.st, r.phi = s.phi, r.windows = s.windows, r.resets = s.resets, r.reserved = 0;
    out[ch] = r;
}

}  // namespace
}  // namespace sdrk

using namespace sdrk;

extern "C" {

void sdr_rds_carrier_opts_default(sdr_rds_carrier_opts* o) {
    if (!o) return;
    o->qshift = 10;
    o->avg_shift = 3;
}

// the derotator's rule for a mode and an options record; `who` names the caller in the text
static int carrier_opts_rule(const char* who, int mode, const sdr_rds_carrier_opts* opts) {
    if (!sdr_rds_mode_ok(mode)) return fail(SDR_E_INVALID, "%s: mode %d has no RDS chain to derotate", who, mode);
    if (opts->qshift < 0 || opts->qshift > 15) return fail(SDR_E_INVALID, "%s: qshift %d is not in 0..15", who, opts->qshift);
    if (opts->avg_shift < 0 || opts->avg_shift > 6)
        return fail(SDR_E_INVALID, "%s: avg_shift %d is not in 0..6", who, opts->avg_shift);
    return SDR_OK;
}

int sdr_rds_carrier_opts_check(int mode, const sdr_rds_carrier_opts* opts) {
    if (!opts) return fail(SDR_E_INVALID, "rds_carrier_opts_check: opts is NULL");
    return carrier_opts_rule("rds_carrier_opts_check", mode, opts);
}

int sdr_rds_carrier_create(sdr_rds_carrier** out, int device, int nch, int mode, const sdr_rds_carrier_opts* opts) {
    if (!out) return fail(SDR_E_INVALID, "rds_carrier_create: out is NULL");
    *out = nullptr;
    if (!opts) return fail(SDR_E_INVALID, "rds_carrier_create: opts is NULL");
    if (nch < 1) return fail(SDR_E_INVALID, "rds_carrier_create: nch %d < 1", nch);
    if (const int r = carrier_opts_rule("rds_carrier_create", mode, opts)) return r;
    sdr_rds_carrier* h = nullptr;
    if (const int r = create_begin(&h, device, "rds_carrier_create")) return r;
    h->nch = nch, h->mode = mode;
    h->opts = *opts;
    hipError_t e = hipSuccess;
    dev_alloc(e, &h->st, (size_t)nch * sizeof(CarState));
    dev_alloc(e, &h->stats, (size_t)nch * sizeof(sdr_rds_carrier_stats));
    create_reset(e, k_carrier_reset, groups256(nch), h->st, nch);
    return create_done(e, h, out, sdr_rds_carrier_destroy, "rds_carrier_create");
}

int sdr_rds_carrier_destroy(sdr_rds_carrier* h) {
    if (!h) return fail(SDR_E_INVALID, "rds_carrier_destroy: null handle");
    return destroy_handle(h, {h->st, h->stats});
}

int sdr_rds_carrier_reset(sdr_rds_carrier* h, void* stream) {
    if (!h) return fail(SDR_E_INVALID, "rds_carrier_reset: null handle");
    return launch_on(h->device, k_carrier_reset, groups256(h->nch), S(stream), h->st, h->nch);
}

int sdr_rds_carrier_rotate(sdr_rds_carrier* h, const float* clean_i, size_t stride_i, const float* clean_q,
                           size_t stride_q, int n, float* out, size_t out_stride, void* stream) {
    if (!h || !clean_i || !clean_q || !out) return fail(SDR_E_INVALID, "rds_carrier_rotate: null argument");
    if (n < 0 || n > SDR_RDS_TRACK_MAX_N)
        return fail(SDR_E_INVALID, "rds_carrier_rotate: n %d is not in 0..%d (SDR_RDS_TRACK_MAX_N)", n, SDR_RDS_TRACK_MAX_N);
    if (stride_i < (size_t)n) return fail(SDR_E_INVALID, "rds_carrier_rotate: stride_i %zu < n = %d", stride_i, n);
    if (stride_q < (size_t)n) return fail(SDR_E_INVALID, "rds_carrier_rotate: stride_q %zu < n = %d", stride_q, n);
    if (out_stride < (size_t)n) return fail(SDR_E_INVALID, "rds_carrier_rotate: out_stride %zu < n = %d", out_stride, n);
    if ((reinterpret_cast<uintptr_t>(clean_i) | reinterpret_cast<uintptr_t>(clean_q) | reinterpret_cast<uintptr_t>(out)) & 3)
        return fail(SDR_E_INVALID, "rds_carrier_rotate: a row is not a float pointer");
    HIP_TRY(hipSetDevice(h->device));
    const float scale = (float)(1 << h->opts.qshift), inv = 1.0f / scale;   // powers of two: exact
    int scale_bits, inv_bits;
    std::memcpy(&scale_bits, &scale, sizeof scale_bits);
    std::memcpy(&inv_bits, &inv, sizeof inv_bits);
    // the 16-byte paths need a row aligned; the kernel looks at its own rows' addresses
    hipLaunchKernelGGL(k_rds_carrier, dim3(h->nch), dim3(64), 0, (hipStream_t)stream, (CarState*)h->st, clean_i, stride_i,
                       clean_q, stride_q, n, out, out_stride, scale_bits, inv_bits, h->opts.avg_shift);
    LAUNCH_CHECK();
    return SDR_OK;
}

int sdr_rds_carrier_stats_read(sdr_rds_carrier* h, sdr_rds_carrier_stats* host_stats, void* stream) {
    if (!h || !host_stats) return fail(SDR_E_INVALID, "rds_carrier_stats_read: null argument");
    if (const int r = launch_on(h->device, k_carrier_stats, groups256(h->nch), S(stream), h->st, h->stats, h->nch)) return r;
    return copy_records(h->stats, host_stats, h->nch, S(stream));
}

}  // extern "C"
