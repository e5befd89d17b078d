// sdr_rds_track.hip -- RDS symbol tracker on MI355X (gfx950): a biphase correlator over the whole bit on a
// bit clock that is carried from call to call and nudged by early/late sums, in place of the per-block
// cdr() of k_rds_bits. No reference counterpart; the definition is in include/sdr_amd.h (sdr_rds_track_*)
// and tests/rds_track_model.py reproduces every bit. One quantisation, then all integer.
//
// k_rds_track, one wave per channel (grid nch, 64 threads), as k_rds_bits and k_rds_groups are laid out:
//   stage     the carried samples and the call's row go to LDS as int32, the row's loads all in flight
//             (16-byte loads where the row is aligned), quantised on the way; a non-finite sample ends the
//             call before any state is touched
//   scan      an in-place inclusive prefix sum I over the carry and the row: per-lane serial runs of an
//             odd length (no bank conflicts), one cross-lane scan of the 64 run totals. A correlator is
//             three reads of it: c(j) = 2 I[j+S-1] - I[j-1] - I[j+B-1]
//   acquire   lane l owns the residues l and l + 64 of E[t mod B] and walks the call's positions of each
//   track     between two decisions nothing depends on anything else: lane 4 b + k takes correlator k
//             (early, on time, late, half) of the round's bit b, a butterfly over the bits gives the four
//             sums, the decision is wave-uniform, __ballot packs the raw bits. A block is about three
//             such rounds, not 37 dependent bits.
// A call longer than TRK_CHUNK samples runs as consecutive chunks through the same LDS: the definition does
// not depend on how the stream is cut, so that is the same result.
// The state is one 640-byte record per channel in HBM; lane 0 writes the scalars back, the lanes the carry
// and the accumulators they own, all with plain vector stores.
#include "stage_host.h"

#include <cstring>

struct sdr_rds_track {
    int device = 0, nch = 0, mode = 0, S = 0;
    sdr_rds_track_opts opts{};
    void* st = nullptr;                   // [nch] TrackState (device)
    sdr_rds_track_stats* stats = nullptr; // [nch] (device), gathered by k_track_stats
};

namespace sdrk {
namespace {

constexpr int TRK_S = 39, TRK_B = 2 * TRK_S;      // mode 0: samples per chip and per bit
constexpr int TRK_T = 16;                         // bits per round: 16 bits x 4 correlators = the 64 lanes
constexpr int TRK_CARRY = SDR_RDS_TRACK_CARRY;
constexpr int TRK_CHUNK = 3072;                   // samples staged at once: a block (2836) in one round of loads
constexpr int TRK_LDS = TRK_CARRY + TRK_CHUNK;    // (x 32767 < 2^31: a chunk's prefix sums fit int32)
static_assert(TRK_CARRY >= TRK_B + TRK_S + 1, "the carry holds the half-bit correlator of the oldest undecided bit");
static_assert((long long)TRK_LDS * 32767 < (1ll << 31), "prefix sums fit int32");
static_assert((long long)TRK_B * 32767 * 64 < (1ll << 31), "the accumulators fit int32 at the longest A and H");
static_assert(SDR_RDS_TRACK_MAX_N == (SDR_MAX_BITS - 1) * (TRK_B - 1) + TRK_B - 1, "bits are at least B - 1 samples apart");

struct TrackHead {                                 // the wave-uniform part, 88 bytes
    int32_t locked;
    int32_t acq_n;                 // acquiring: samples consumed since the stream (re)started
    int32_t ta;                    // acquiring: the next position that adds to E
    int32_t d;                     // tracking: the next bit's start minus the samples consumed (>= -B)
    int32_t phase;                 // tracking: the next bit's start mod B
    int32_t prev, cnt;             // the last raw bit, bits in the round so far
    int32_t early, on, late, half; // the round's sums
    int32_t hr, hon, hhalf;        // the half check: rounds so far, its sums
    uint32_t level, bits, moves, half_moves, resets, acquired;
    int32_t pad[2];
};
struct alignas(64) TrackState {                   // 640 bytes
    TrackHead h;
    int32_t E[TRK_B];              // acquisition accumulators
    int16_t carry[TRK_CARRY];      // the last quantised samples, the newest last
};
static_assert(sizeof(TrackState) == 640, "TrackState is ten 64-byte lines");

__device__ __forceinline__ int quant(float x, int qshift_scale_bits) {
    // rint(clamp(x * 2^k, +-32767)): the clamp first, so that an overflowing product is clamped too
    const float y = fminf(fmaxf(x * __int_as_float(qshift_scale_bits), -32767.0f), 32767.0f);
    return __float2int_rn(y);
}
__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

__device__ __forceinline__ int corr_at(const int* I, int j) {   // c of the bit that starts at buffer index j >= 1
    return 2 * I[j + TRK_S - 1] - I[j - 1] - I[j + TRK_B - 1];
}

__device__ __forceinline__ void restart(TrackHead& s) {        // back to acquiring; the counters stay
    s.locked = 0, s.acq_n = 0, s.ta = 0, s.d = 0, s.phase = 0, s.prev = 0, s.cnt = 0;
    s.early = s.on = s.late = s.half = 0;
    s.hr = s.hon = s.hhalf = 0;
    s.level = 0;
}

// SOFT: the on-time lanes also write |c(t)| >> 6 of their raw decision (sdr_rds_track_bits_soft); the default
// instantiation has none of it
template <bool SOFT>
__global__ __launch_bounds__(64) void k_rds_track(TrackState* __restrict__ st_all, const float* __restrict__ x,
                                                  size_t x_stride, int n, int32_t* __restrict__ nbits,
                                                  uint8_t* __restrict__ bits, size_t bits_stride, int scale_bits,
                                                  int A, int H_rounds, uint16_t* __restrict__ soft, size_t soft_stride) {
    __shared__ int I[TRK_LDS + 4];
    const int ch = blockIdx.x, lane = threadIdx.x;
    TrackState* sp = st_all + ch;
    const float* xc = x + (size_t)ch * x_stride;
    uint8_t* bo = bits + (size_t)ch * bits_stride;
    if (n <= 0) {
        if (lane == 0) nbits[ch] = 0;
        return;
    }
    TrackHead s = sp->h;           // wave-uniform (E and carry are read where they are used)
    const bool vec4 = (reinterpret_cast<uintptr_t>(xc) & 15) == 0;
    // ---- a call of more than one chunk: look for a non-finite sample before any of it is used
    bool bad = false;
    if (n > TRK_CHUNK) {
        for (int i = lane; i < n; i += 64) bad |= !finite_bits(xc[i]);
        bad = __any(bad);
    }
    // ---- the carry in front
    for (int i = lane; i < TRK_CARRY; i += 64) I[i] = s.locked || s.acq_n ? (int)sp->carry[i] : 0;
    int E0 = 0, E1 = 0;            // lane l owns E[l] and E[l + 64]
    if (!s.locked) {
        E0 = sp->E[lane];
        if (lane + 64 < TRK_B) E1 = sp->E[lane + 64];
    }
    int nb = 0;
    for (int c0 = 0; c0 < n && !bad; c0 += TRK_CHUNK) {
        const int m = min(TRK_CHUNK, n - c0);
        const float* xr = xc + c0;                 // c0 is a multiple of 4: the alignment of xc holds
        int* q = I + TRK_CARRY;
        // ---- stage and quantise: every load of a round in flight, then the LDS writes
        int i_tail = 0;
        if (vec4) {
            constexpr int U4 = 12;
            const int n4 = m >> 2;
            for (int q0 = lane; q0 < n4; q0 += 64 * U4) {
                // unconditional at a clamped index (lanes past the row rewrite its last vector)
                float4 v[U4];
#pragma unroll
                for (int u = 0; u < U4; u++) v[u] = reinterpret_cast<const float4*>(xr)[min(q0 + 64 * u, n4 - 1)];
#pragma unroll
                for (int u = 0; u < U4; u++) {
                    const int k = 4 * min(q0 + 64 * u, n4 - 1);
                    bad |= !(finite_bits(v[u].x) && finite_bits(v[u].y) && finite_bits(v[u].z) && finite_bits(v[u].w));
                    q[k] = quant(v[u].x, scale_bits), q[k + 1] = quant(v[u].y, scale_bits);
                    q[k + 2] = quant(v[u].z, scale_bits), q[k + 3] = quant(v[u].w, scale_bits);
                }
            }
            i_tail = n4 * 4;
        }
        constexpr int U = 8;
        for (int i0 = i_tail + lane; i0 < m; i0 += 64 * U) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; u++) v[u] = xr[min(i0 + 64 * u, m - 1)];
#pragma unroll
            for (int u = 0; u < U; u++) {
                bad |= !finite_bits(v[u]);
                q[min(i0 + 64 * u, m - 1)] = quant(v[u], scale_bits);
            }
        }
        bad = __any(bad);
        if (bad) break;
        __syncthreads();
        // ---- inclusive prefix sum of I[0 .. L) in place
        const int L = TRK_CARRY + m;
        const int R = ((L + 63) >> 6) | 1;         // odd: lanes R apart hit different banks
        const int r0 = min(lane * R, L), r1 = min(r0 + R, L);
        int run = 0;
        for (int i = r0; i < r1; i++) run += I[i];
        int incl = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        int acc = incl - run;                      // the sum of the runs before this lane's
        // the carry for the next chunk or call: the last TRK_CARRY samples, read before the scan overwrites them
        int cq0 = 0, cq1 = 0;
        {
            const int a = L - TRK_CARRY + lane, b = a + 64;
            cq0 = I[a];
            if (lane + 64 < TRK_CARRY) cq1 = I[b];
        }
        __syncthreads();
        for (int i = r0; i < r1; i++) {
            acc += I[i];
            I[i] = acc;
        }
        __syncthreads();
        // ---- acquire: position p of the stream is buffer index p - acq_n + TRK_CARRY
        if (!s.locked) {
            const int AB = A * TRK_B;
            const int hi = min(s.acq_n + m - TRK_B, AB - 1);
            const int shift = TRK_CARRY - s.acq_n;
            const int ta_mod = s.ta % TRK_B;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int r = lane + 64 * h;
                if (r >= TRK_B) break;
                int e = h ? E1 : E0;
                for (int t = s.ta + (r - ta_mod + TRK_B) % TRK_B; t <= hi; t += TRK_B) e += abs(corr_at(I, t + shift));
                if (h) E1 = e;
                else E0 = e;
            }
            if (hi >= s.ta) s.ta = hi + 1;
            if (s.ta == AB) {
                // the first maximum: the largest (value, B - 1 - residue)
                long long key = ((long long)E0 << 8) | (long long)(TRK_B - 1 - lane);
                if (lane + 64 < TRK_B) {
                    const long long k1 = ((long long)E1 << 8) | (long long)(TRK_B - 1 - (lane + 64));
                    key = k1 > key ? k1 : key;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const long long other = __shfl_xor(key, o);
                    key = other > key ? other : key;
                }
                s.phase = TRK_B - 1 - (int)(key & 0xFF);
                s.locked = 1;
                s.acquired++;
                s.d = AB + s.phase - s.acq_n;
                s.prev = 0, s.cnt = 0;
                s.early = s.on = s.late = s.half = 0;
                s.hr = s.hon = s.hhalf = 0;
            }
        }
        // ---- track: rounds of up to T bits, every lane one correlator of one bit
        if (s.locked) {
            int j = s.d + TRK_CARRY;               // the next bit's start as a buffer index (>= CARRY - B)
            const int bit = lane >> 2, kind = lane & 3;
            const int off = kind == 0 ? -1 : kind == 1 ? 0 : kind == 2 ? 1 : -TRK_S;
            while (j + TRK_B < L) {
                const int k = min((L - 1 - TRK_B - j) / TRK_B + 1, TRK_T - s.cnt);   // bits decided in this round
                const bool valid = bit < k;
                const int jj = j + bit * TRK_B + off;
                const int v = valid && jj >= 1 ? corr_at(I, jj) : 0;
                int a = abs(v);
#pragma unroll
                for (int o = 4; o < 64; o <<= 1) a += __shfl_xor(a, o);
                const unsigned long long raw = __ballot(valid && kind == 1 && v > 0);
                if (valid && kind == 1) {
                    const int r = v > 0 ? 1 : 0;
                    const int before = bit == 0 ? s.prev : (int)((raw >> (4 * (bit - 1) + 1)) & 1);
                    if (nb + bit < SDR_MAX_BITS) {
                        bo[nb + bit] = (uint8_t)(r ^ before);
                        if constexpr (SOFT) soft[(size_t)ch * soft_stride + nb + bit] = (uint16_t)(abs(v) >> 6);
                    }
                }
                s.prev = (int)((raw >> (4 * (k - 1) + 1)) & 1);
                s.early += __shfl(a, 0), s.on += __shfl(a, 1), s.late += __shfl(a, 2), s.half += __shfl(a, 3);
                nb += k;
                s.cnt += k;
                j += k * TRK_B;
                if (s.cnt < TRK_T) break;          // the call ends inside the round
                s.level = (uint32_t)s.on;
                s.hon += s.on, s.hhalf += s.half;
                s.hr++;
                bool jump = false;
                if (s.hr == H_rounds) {
                    jump = s.hhalf > s.hon;
                    s.hr = s.hon = s.hhalf = 0;
                }
                int step = 0;
                if (jump) step = TRK_S, s.half_moves++;
                else if (s.early > s.on && s.early >= s.late) step = -1, s.moves++;
                else if (s.late > s.on) step = 1, s.moves++;
                j += step;
                s.phase = (s.phase + step + TRK_B) % TRK_B;
                s.cnt = 0;
                s.early = s.on = s.late = s.half = 0;
            }
            s.d = j - TRK_CARRY - m;               // against the samples consumed after this chunk
        } else {
            s.acq_n += m;
        }
        // ---- the carry moves to the front for the next chunk (and is what the state keeps)
        __syncthreads();
        I[lane] = cq0;
        if (lane + 64 < TRK_CARRY) I[lane + 64] = cq1;
        __syncthreads();
    }
    if (bad) {                     // uniform: nothing of the call is used, the stream starts again
        restart(s);
        s.resets++;
        sp->E[lane] = 0;
        if (lane + 64 < TRK_B) sp->E[lane + 64] = 0;
        if (lane == 0) {
            sp->h = s;
            nbits[ch] = SDR_NBITS_POISONED;
        }
        return;
    }
    s.bits += (uint32_t)nb;
    sp->carry[lane] = (int16_t)I[lane];
    if (lane + 64 < TRK_CARRY) sp->carry[lane + 64] = (int16_t)I[lane + 64];
    if (!s.locked) {
        sp->E[lane] = E0;
        if (lane + 64 < TRK_B) sp->E[lane + 64] = E1;
    }
    if (lane == 0) {
        sp->h = s;
        nbits[ch] = nb;
    }
}

__global__ void k_track_reset(TrackState* st, int nch) {   // all zero: acquiring, an empty stream, no counts
    constexpr size_t W = sizeof(TrackState) / sizeof(uint32_t);
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)nch * W) reinterpret_cast<uint32_t*>(st)[i] = 0u;
}

__global__ void k_track_stats(const TrackState* st, sdr_rds_track_stats* out, int nch) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= nch) return;
    const TrackHead& s = st[ch].h;
    sdr_rds_track_stats r;
    r.locked = (uint32_t)s.locked, r.phase = s.locked ? (uint32_t)s.phase : 0u, r.bits = s.bits, r.moves = s.moves;
    r.half_moves = s.half_moves, r.resets = s.resets, r.level = s.level, r.acquired = s.acquired;
    out[ch] = r;
}

unsigned reset_grid(int nch) { return (unsigned)(((size_t)nch * (sizeof(TrackState) / 4) + 255) / 256); }

}  // namespace
}  // namespace sdrk

using namespace sdrk;

extern "C" {

void sdr_rds_track_opts_default(sdr_rds_track_opts* o) {
    if (!o) return;
    o->qshift = 10;
    o->acquire_bits = 32;
    o->half_bits = 64;
}

// the tracker's rule for a mode and an options record; `who` names the caller in the text
static int track_opts_rule(const char* who, int mode, const sdr_rds_track_opts* opts, sdr_info* in) {
    if (!sdr_rds_mode_ok(mode)) return fail(SDR_E_INVALID, "%s: mode %d has no 1187.5 bit/s clock", who, mode);
    if (opts->qshift < 0 || opts->qshift > 15) return fail(SDR_E_INVALID, "%s: qshift %d is not in 0..15", who, opts->qshift);
    if (opts->acquire_bits < 1 || opts->acquire_bits > 64)
        return fail(SDR_E_INVALID, "%s: acquire_bits %d is not in 1..64", who, opts->acquire_bits);
    if (opts->half_bits < SDR_RDS_TRACK_T || opts->half_bits > 64 || opts->half_bits % SDR_RDS_TRACK_T)
        return fail(SDR_E_INVALID, "%s: half_bits %d is not a multiple of %d in %d..64", who, opts->half_bits,
                    SDR_RDS_TRACK_T, SDR_RDS_TRACK_T);
    if (mode_info(in, 1, mode, 1) != SDR_OK || in->symbol_Fs != TRK_S)
        return fail(SDR_E_INVALID, "%s: mode %d is not at %d samples a chip", who, mode, TRK_S);
    return SDR_OK;
}

int sdr_rds_track_opts_check(int mode, const sdr_rds_track_opts* opts) {
    if (!opts) return fail(SDR_E_INVALID, "rds_track_opts_check: opts is NULL");
    sdr_info in;
    return track_opts_rule("rds_track_opts_check", mode, opts, &in);
}

int sdr_rds_track_create(sdr_rds_track** out, int device, int nch, int mode, const sdr_rds_track_opts* opts) {
    if (!out) return fail(SDR_E_INVALID, "rds_track_create: out is NULL");
    *out = nullptr;
    if (!opts) return fail(SDR_E_INVALID, "rds_track_create: opts is NULL");
    if (nch < 1) return fail(SDR_E_INVALID, "rds_track_create: nch %d < 1", nch);
    sdr_info in;
    if (const int r = track_opts_rule("rds_track_create", mode, opts, &in)) return r;
    sdr_rds_track* t = nullptr;
    if (const int r = create_begin(&t, device, "rds_track_create")) return r;
    t->nch = nch, t->mode = mode, t->S = in.symbol_Fs;
    t->opts = *opts;
    hipError_t e = hipSuccess;
    dev_alloc(e, &t->st, (size_t)nch * sizeof(TrackState));
    dev_alloc(e, &t->stats, (size_t)nch * sizeof(sdr_rds_track_stats));
    create_reset(e, k_track_reset, reset_grid(nch), t->st, nch);
    return create_done(e, t, out, sdr_rds_track_destroy, "rds_track_create");
}

int sdr_rds_track_destroy(sdr_rds_track* t) {
    if (!t) return fail(SDR_E_INVALID, "rds_track_destroy: null handle");
    return destroy_handle(t, {t->st, t->stats});
}

int sdr_rds_track_reset(sdr_rds_track* t, void* stream) {
    if (!t) return fail(SDR_E_INVALID, "rds_track_reset: null handle");
    return launch_on(t->device, k_track_reset, reset_grid(t->nch), S(stream), t->st, t->nch);
}

static int track_call(sdr_rds_track* t, const float* clean_dev, size_t clean_stride, int n, int32_t* nbits_dev,
                      uint8_t* bits_dev, size_t bits_stride, bool with_soft, uint16_t* soft_dev, size_t soft_stride,
                      void* stream) {
    if (!t || !clean_dev || !nbits_dev || !bits_dev) return fail(SDR_E_INVALID, "rds_track_bits: null argument");
    if (with_soft && !soft_dev) return fail(SDR_E_INVALID, "rds_track_bits_soft: soft_dev is NULL");
    if (with_soft && soft_stride < SDR_MAX_BITS)
        return fail(SDR_E_INVALID, "rds_track_bits_soft: soft_stride %zu < SDR_MAX_BITS = %d", soft_stride, SDR_MAX_BITS);
    if (with_soft && (reinterpret_cast<uintptr_t>(soft_dev) & 1))
        return fail(SDR_E_INVALID, "rds_track_bits_soft: soft_dev is not a uint16 pointer");
    if (n < 0 || n > SDR_RDS_TRACK_MAX_N)
        return fail(SDR_E_INVALID, "rds_track_bits: n %d is not in 0..%d (a call holds at most SDR_MAX_BITS bits)", n,
                    SDR_RDS_TRACK_MAX_N);
    if (clean_stride < (size_t)n) return fail(SDR_E_INVALID, "rds_track_bits: clean_stride %zu < n = %d", clean_stride, n);
    if (bits_stride < SDR_MAX_BITS)
        return fail(SDR_E_INVALID, "rds_track_bits: bits_stride %zu < SDR_MAX_BITS = %d", bits_stride, SDR_MAX_BITS);
    if (reinterpret_cast<uintptr_t>(clean_dev) & 3) return fail(SDR_E_INVALID, "rds_track_bits: clean_dev is not a float pointer");
    HIP_TRY(hipSetDevice(t->device));
    const float scale = (float)(1 << t->opts.qshift);
    int scale_bits;
    std::memcpy(&scale_bits, &scale, sizeof scale_bits);
    // the 16-byte staging path needs every row aligned; the kernel looks at its own row's address
    if (with_soft)
        hipLaunchKernelGGL(k_rds_track<true>, dim3(t->nch), dim3(64), 0, (hipStream_t)stream, (TrackState*)t->st, clean_dev,
                           clean_stride, n, nbits_dev, bits_dev, bits_stride, scale_bits, t->opts.acquire_bits,
                           t->opts.half_bits / SDR_RDS_TRACK_T, soft_dev, soft_stride);
    else
        hipLaunchKernelGGL(k_rds_track<false>, dim3(t->nch), dim3(64), 0, (hipStream_t)stream, (TrackState*)t->st, clean_dev,
                           clean_stride, n, nbits_dev, bits_dev, bits_stride, scale_bits, t->opts.acquire_bits,
                           t->opts.half_bits / SDR_RDS_TRACK_T, (uint16_t*)nullptr, (size_t)0);
    LAUNCH_CHECK();
    return SDR_OK;
}

int sdr_rds_track_bits(sdr_rds_track* t, const float* clean_dev, size_t clean_stride, int n, int32_t* nbits_dev,
                       uint8_t* bits_dev, size_t bits_stride, void* stream) {
    return track_call(t, clean_dev, clean_stride, n, nbits_dev, bits_dev, bits_stride, false, nullptr, 0, stream);
}

int sdr_rds_track_bits_soft(sdr_rds_track* t, const float* clean_dev, size_t clean_stride, int n, int32_t* nbits_dev,
                            uint8_t* bits_dev, size_t bits_stride, uint16_t* soft_dev, size_t soft_stride, void* stream) {
    return track_call(t, clean_dev, clean_stride, n, nbits_dev, bits_dev, bits_stride, true, soft_dev, soft_stride, stream);
}

int sdr_rds_track_stats_read(sdr_rds_track* t, sdr_rds_track_stats* host_stats, void* stream) {
    if (!t || !host_stats) return fail(SDR_E_INVALID, "rds_track_stats_read: null argument");
    if (const int r = launch_on(t->device, k_track_stats, groups256(t->nch), S(stream), t->st, t->stats, t->nch)) return r;
    return copy_records(t->stats, host_stats, t->nch, S(stream));
}

}  // extern "C"
