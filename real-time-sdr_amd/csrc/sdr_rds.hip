// sdr_rds.hip -- RDS group decoder on MI355X (gfx950): block synchronisation with a flywheel, +-1 bit slip
// recovery and burst-error correction over the bits k_rds_bits wrote. No reference counterpart; the
// definition is in include/sdr_amd.h (sdr_rds_*) and tests/rds_model.py reproduces every bit. All integer.
//
// k_rds_groups, one wave per channel (grid nch, 64 threads), as k_rds_bits is laid out:
//   parallel  the call's bits become four 64-bit lane masks by __ballot; with the 64-bit history in front
//             they are one 320-bit string. Window q (0 <= q < nb + 2) is the 26 bits that end at the call's
//             bit q - 2: lane l takes the windows q = l + 64 t, t < 5, and computes each syndrome as ten
//             masked-popcount parities against the rows of the parity-check matrix (no division). The
//             syndromes go to LDS; the windows that match an offset word become five hit masks by __ballot.
//   serial    a wave-uniform walk over the call: while synchronised it jumps from judgement point to
//             judgement point (at most 11 in 256 bits), while not it jumps from hit to hit by find-first-set
//             on the hit masks, and it changes mode in the middle of a call exactly where the model does.
//             All that it reads is the absolute state, so the cut of the stream into calls does not matter.
// The state is one 128-byte record per channel in HBM, written back by lane 0 with plain vector stores;
// the correction table (1024 x u32) is read on the failing-block path only.
#include "stage_host.h"

#include <cstring>

struct sdr_rds_dec {
    int device = 0, nch = 0, max_burst = 0, loss_blocks = 0;
    void* st = nullptr;             // [nch] RdsState (device)
    uint32_t* tab = nullptr;        // [1024] correction table (device)
    sdr_rds_group* groups = nullptr;   // [nch][SDR_RDS_MAX_GROUPS] (device)
    int32_t* ngroups = nullptr;     // [nch] (device)
    sdr_rds_stats* stats = nullptr; // [nch] (device), gathered by k_rds_stats
    // a handle of sdr_rds_dec_create_soft
    bool soft = false;
    int soft_bits = 0;
    uint16_t* hist = nullptr;       // [nch][SDR_RDS_SOFT_HISTORY] the soft values of the last bits consumed (device)
    sdr_rds_soft_stats* sstats = nullptr;   // [nch] (device), gathered by k_rds_soft_stats
};

namespace sdrk {
namespace {

constexpr uint32_t M26 = (1u << 26) - 1;
constexpr int NWIN = 320;          // windows a call can look at: 5 per lane
constexpr uint32_t OFFW[5] = {0x0FC, 0x198, 0x168, 0x350, 0x1B4};   // A, B, C, C', D

struct alignas(64) RdsState {      // 128 bytes
    uint64_t sr;                   // the latest 64 bits, the newest in bit 0
    uint64_t n;                    // bits consumed since the last reset
    uint64_t judge_at;             // synchronised: the bit index of the next judgement
    uint64_t pend_pos;             // the pending hit's bit index
    uint64_t words;                // the group in assembly: word b in bits 16 b .. 16 b + 15
    uint8_t ok, corrected, flags, synced;
    int32_t expect, bad_run, pend_idx;   // pend_idx < 0: no pending hit
    uint32_t good, ncorrected, bad, slips, acquired, lost, groups;
    uint32_t soft_blocks, soft_flips;    // the soft step's counters (zero on a handle without it)
    uint32_t pad[9];
};
static_assert(sizeof(RdsState) == 128, "RdsState is two 64-byte lines");

struct ParityRows {
    uint32_t r[10];                // syndrome bit k = parity(w26 & r[k])
};

// the 26 bits that end at string position p (position 0 = the oldest history bit, the first of a word in
// its bit 63); wd[0] = 0 stands in front of the history
__device__ __forceinline__ uint64_t tail_bits(const uint64_t* wd, int p) {
    const int k = (p >> 6) + 1, sh = 63 - (p & 63);
    const uint64_t lo = wd[k], hi = wd[k - 1];
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

__device__ __forceinline__ uint32_t syn_of(uint32_t w, const ParityRows& pr) {
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 10; k++) s |= (uint32_t)(__popc(w & pr.r[k]) & 1) << k;
    return s;
}

// the offset (0..4) of block index blk that the syndrome matches, C before C'; -1: none
__device__ __forceinline__ int match_block(uint32_t s, int blk) {
    if (blk == 2) return s == OFFW[2] ? 2 : (s == OFFW[3] ? 3 : -1);
    const int o = blk == 3 ? 4 : blk;
    return s == OFFW[o] ? o : -1;
}

constexpr int SOFT_WIN = 27;       // raw decisions behind the 26 diff bits of a word
constexpr int SOFT_HIST = SDR_RDS_SOFT_HISTORY;
static_assert(SOFT_HIST >= SOFT_WIN + 1, "the history holds a window that ends one bit before the call's first");

// the diff bits of the nominal word that flipping window raw p (0 = the oldest) toggles: r and r + 1, clipped
__device__ __forceinline__ uint32_t soft_toggle(int p) { return ((3u << 26) >> (p + 1)) & M26; }

// The soft step of a failing block (wave-parallel, every lane returns the same): sv[0 .. 26] are the window's
// soft values, the oldest first. Lanes 0..26 rank them by counting smaller (soft, position) pairs, the L
// lowest ranks publish their toggle mask and soft, lane m builds e(m) and w(m) and the syndrome of
// nominal ^ e(m), and a wave minimum of w * 64 + m (< 2^25) over the matching lanes picks the winner.
// Returns e of the winner (never 0) and its offset and m, or 0.
__device__ __forceinline__ uint32_t soft_search(const uint16_t* sv, uint32_t* cmask, uint32_t* csoft, uint32_t nominal,
                                                int expect, int L, const ParityRows& pr, int lane, int* o_out, int* m_out) {
    if (lane < SOFT_WIN) {
        const uint32_t mine = ((uint32_t)sv[lane] << 5) | (uint32_t)lane;
        int rank = 0;
        for (int q = 0; q < SOFT_WIN; q++) rank += (((uint32_t)sv[q] << 5) | (uint32_t)q) < mine ? 1 : 0;
        if (rank < L) {
            cmask[rank] = soft_toggle(lane);
            csoft[rank] = sv[lane];
        }
    }
    __syncthreads();
    uint32_t e = 0, w = 0;
    for (int j = 0; j < L; j++)
        if ((lane >> j) & 1) e ^= cmask[j], w += csoft[j];
    int o = -1;
    if (lane >= 1 && lane < (1 << L)) o = match_block(syn_of(nominal ^ e, pr), expect);
    uint32_t key = o >= 0 ? (w << 6) | (uint32_t)lane : 0xFFFFFFFFu;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)key, d);
        key = other < key ? other : key;
    }
    __syncthreads();               // cmask and csoft are free for the next judgement
    if (key == 0xFFFFFFFFu) return 0;
    const int m = (int)(key & 63u);
    *m_out = m;
    *o_out = __shfl(o, m);
    return (uint32_t)__shfl((int)e, m);
}

// SOFT: the soft step between the late alignment and the burst table, the call's soft values and the history
// in LDS (sdr_rds_groups_soft); the default instantiation has none of it
template <bool SOFT>
__global__ __launch_bounds__(64) void k_rds_groups(RdsState* __restrict__ st_all, const int32_t* __restrict__ nbits,
                                                   const uint8_t* __restrict__ bits, size_t bits_stride,
                                                   const uint32_t* __restrict__ tab, sdr_rds_group* __restrict__ groups,
                                                   int32_t* __restrict__ ngroups, int loss_blocks, ParityRows pr,
                                                   const uint16_t* __restrict__ soft, size_t soft_stride,
                                                   uint16_t* __restrict__ hist_all, int soft_bits) {
    __shared__ uint64_t wd[6];
    __shared__ uint16_t syn[NWIN];
    __shared__ uint16_t sv[SOFT ? SOFT_HIST + SDR_MAX_BITS : 1];   // the history, then the call's soft values
    __shared__ uint32_t cmask[SOFT ? 8 : 1], csoft[SOFT ? 8 : 1];
    const int ch = blockIdx.x, lane = threadIdx.x;
    RdsState* sp = st_all + ch;
    const int nb = nbits[ch];
    int ng = 0;
    if (nb == SDR_NBITS_POISONED) {
        if (lane == 0) {
            if (sp->synced) {
                sp->synced = 0;
                sp->lost = sp->lost + 1;
            }
            sp->pend_idx = -1;
            sp->words = 0;
            sp->ok = sp->corrected = sp->flags = 0;
            ngroups[ch] = 0;
        }
        return;
    }
    if (nb < 0 || nb > SDR_MAX_BITS) {
        if (lane == 0) ngroups[ch] = 0;
        return;
    }
    RdsState s = *sp;   // wave-uniform
    const uint8_t* row = bits + (size_t)ch * bits_stride;
    // ---- the bit string: wd[1] = history, wd[2..5] = the call's bits, first bit in bit 63
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int j = 64 * t + lane;
        const int b = j < nb ? (row[j] & 1) : 0;
        const uint64_t m = __ballot(b);
        if (lane == 0) wd[2 + t] = __brevll(m);
    }
    if (lane == 0) {
        wd[0] = 0;
        wd[1] = s.sr;
    }
    if constexpr (SOFT) {
        const uint16_t* srow = soft + (size_t)ch * soft_stride;
        if (lane < SOFT_HIST) sv[lane] = hist_all[(size_t)ch * SOFT_HIST + lane];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int j = 64 * t + lane;
            sv[SOFT_HIST + j] = j < nb ? srow[j] : (uint16_t)0;
        }
    }
    __syncthreads();
    // ---- syndromes of the windows q = lane + 64 t (ending at string position q + 62), hit masks
    const int nwin = nb + 2;
    uint64_t hit[5];
#pragma unroll
    for (int t = 0; t < 5; t++) {
        const int q = 64 * t + lane;
        uint32_t sy = 0x3FF + 1;   // no syndrome: matches nothing
        if (q < nwin) sy = syn_of((uint32_t)tail_bits(wd, q + 62) & M26, pr);
        syn[q] = (uint16_t)sy;
        const bool h = sy == OFFW[0] || sy == OFFW[1] || sy == OFFW[2] || sy == OFFW[3] || sy == OFFW[4];
        hit[t] = __ballot(h);
    }
    __syncthreads();
    // ---- the walk (wave-uniform): j is the call's bit index, q = j + 2 its latest-26 window
    const uint64_t n0 = s.n;
    int pos = 0;
    while (pos < nb) {
        if (s.synced) {
            const uint64_t rel = s.judge_at - n0;     // >= pos: a judgement is never behind the walk
            if (rel >= (uint64_t)nb) break;
            const int j = (int)rel;
            const uint64_t i = n0 + (uint64_t)j;
            const uint32_t s_late = syn[j + 2], s_nom = syn[j + 1], s_early = syn[j];
            int o, wq = j + 1, corr = 0;
            uint32_t fix = 0;
            uint64_t next = i + 26;
            int verdict = 0;                          // 0 good, 1 corrected, 2 bad
            if ((o = match_block(s_nom, s.expect)) >= 0) {
            } else if ((o = match_block(s_early, s.expect)) >= 0) {
                wq = j;
                next = i + 25;
                s.slips++;
            } else if ((o = match_block(s_late, s.expect)) >= 0) {
                wq = j + 2;
                next = i + 27;
                s.slips++;
            } else {
                verdict = 2;
                if constexpr (SOFT) {
                    if (soft_bits > 0) {
                        // the window's raws i-27 .. i-1 are the call's j-27 .. j-1: sv[HIST + j - 27 ..]
                        const uint32_t nominal = (uint32_t)tail_bits(wd, j + 1 + 62) & M26;
                        int so = -1, sm = 0;
                        fix = soft_search(sv + SOFT_HIST - SOFT_WIN + j, cmask, csoft, nominal, s.expect, soft_bits, pr, lane,
                                          &so, &sm);
                        if (fix) {
                            verdict = 1, corr = 1, o = so;
                            s.soft_blocks++;
                            s.soft_flips += (uint32_t)__popc((uint32_t)sm);
                            s.flags |= (uint8_t)(1u << (SDR_RDS_GROUP_SOFT_SHIFT + s.expect));
                        }
                    }
                }
                if (!fix) {
                    const int o0 = s.expect == 3 ? 4 : s.expect;
                    fix = tab[(s_nom ^ OFFW[o0]) & 0x3FF];
                    o = o0;
                    if (!fix && s.expect == 2) {
                        fix = tab[(s_nom ^ OFFW[3]) & 0x3FF];
                        o = 3;
                    }
                    if (fix) verdict = 1, corr = 1;
                }
            }
            s.judge_at = next;
            pos = j + 1;
            if (verdict == 2) {
                s.bad++;
                s.bad_run++;
                if (s.bad_run == loss_blocks) {
                    s.synced = 0;
                    s.lost++;
                    s.pend_idx = -1;
                    s.words = 0;
                    s.ok = s.corrected = s.flags = 0;
                    continue;                         // the search starts with the next bit
                }
            } else {
                const uint32_t word = ((uint32_t)tail_bits(wd, wq + 62) & M26) ^ fix;
                s.words |= (uint64_t)(word >> 10) << (16 * s.expect);
                s.ok |= (uint8_t)(1u << s.expect);
                if (corr) {
                    s.ncorrected++;
                    s.corrected |= (uint8_t)(1u << s.expect);
                } else {
                    s.good++;
                    s.bad_run = 0;
                }
                if (o == 3) s.flags |= SDR_RDS_GROUP_CPRIME;
            }
            // end of block
            if (s.expect == 3) {
                if (s.ok) {
                    s.groups++;
                    if (lane == 0 && ng < SDR_RDS_MAX_GROUPS) {
                        sdr_rds_group g;
                        g.w[0] = (uint16_t)s.words, g.w[1] = (uint16_t)(s.words >> 16), g.w[2] = (uint16_t)(s.words >> 32),
                        g.w[3] = (uint16_t)(s.words >> 48);
                        g.ok = s.ok, g.corrected = s.corrected, g.flags = s.flags, g.reserved = 0;
                        g.bits = (uint32_t)(i + 1);
                        groups[(size_t)ch * SDR_RDS_MAX_GROUPS + ng] = g;
                    }
                    ng++;
                }
                s.words = 0;
                s.ok = s.corrected = s.flags = 0;
            }
            s.expect = (s.expect + 1) & 3;
            // the next judgement is at least 25 bits on
            const uint64_t nrel = s.judge_at - n0;
            pos = nrel >= (uint64_t)nb ? nb : (int)nrel;
        } else {
            // the first hit at or after pos, from the 26th bit since the reset on
            int j0 = pos;
            if (n0 < 25 && (uint64_t)j0 < 25 - n0) j0 = (int)(25 - n0);
            int q = j0 + 2, found = -1;
            while (q < nwin) {
                const int t = q >> 6;
                uint64_t m = t == 0 ? hit[0] : t == 1 ? hit[1] : t == 2 ? hit[2] : t == 3 ? hit[3] : hit[4];
                m &= ~(uint64_t)0 << (q & 63);
                if (m) {
                    found = 64 * t + __ffsll((unsigned long long)m) - 1;
                    break;
                }
                q = 64 * (t + 1);
            }
            if (found < 0 || found >= nwin) break;
            const int j = found - 2;
            const uint64_t i = n0 + (uint64_t)j;
            const uint32_t sy = syn[found];
            const int o = sy == OFFW[0] ? 0 : sy == OFFW[1] ? 1 : sy == OFFW[2] ? 2 : sy == OFFW[3] ? 3 : 4;
            const int idx = o == 4 ? 3 : (o == 3 ? 2 : o);
            pos = j + 1;
            bool acquire = false;
            if (s.pend_idx >= 0) {
                const uint64_t d = i - s.pend_pos;
                if (d >= 26 && d <= 104 && d % 26 == 0 && ((s.pend_idx + (int)(d / 26)) & 3) == idx) acquire = true;
            }
            if (!acquire) {
                s.pend_pos = i;
                s.pend_idx = idx;
                continue;
            }
            s.acquired++;
            s.bad_run = 0;
            s.synced = 1;
            s.expect = idx;
            s.good++;
            s.pend_idx = -1;
            s.words = 0;
            s.ok = s.corrected = 0;
            s.flags = o == 3 ? SDR_RDS_GROUP_CPRIME : 0;
            s.words = (uint64_t)(((uint32_t)tail_bits(wd, found + 62) & M26) >> 10) << (16 * idx);
            s.ok = (uint8_t)(1u << idx);
            if (idx == 3) {
                s.groups++;
                if (lane == 0 && ng < SDR_RDS_MAX_GROUPS) {
                    sdr_rds_group g;
                    g.w[0] = (uint16_t)s.words, g.w[1] = (uint16_t)(s.words >> 16), g.w[2] = (uint16_t)(s.words >> 32),
                        g.w[3] = (uint16_t)(s.words >> 48);
                    g.ok = s.ok, g.corrected = 0, g.flags = 0, g.reserved = 0;
                    g.bits = (uint32_t)(i + 1);
                    groups[(size_t)ch * SDR_RDS_MAX_GROUPS + ng] = g;
                }
                ng++;
                s.words = 0;
                s.ok = s.flags = 0;
            }
            s.expect = (idx + 1) & 3;
            s.judge_at = i + 27;
        }
    }
    // ---- the new history: the 64 bits that end at the call's last bit
    s.sr = tail_bits(wd, 63 + nb);
    s.n = n0 + (uint64_t)nb;
    if constexpr (SOFT) {          // the soft values of the last bits consumed; nb = 0 rewrites what was there
        if (lane < SOFT_HIST) hist_all[(size_t)ch * SOFT_HIST + lane] = sv[nb + lane];
    }
    if (lane == 0) {
        *sp = s;
        ngroups[ch] = ng < SDR_RDS_MAX_GROUPS ? ng : SDR_RDS_MAX_GROUPS;
    }
}

__global__ void k_rds_reset(RdsState* st, sdr_rds_group* groups, int32_t* ngroups, int nch, uint16_t* hist) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= nch) return;
    if (hist)
        for (int k = 0; k < SOFT_HIST; k++) hist[(size_t)ch * SOFT_HIST + k] = 0;
    RdsState z;
    memset(&z, 0, sizeof z);
    z.pend_idx = -1;
    st[ch] = z;
    ngroups[ch] = 0;
    sdr_rds_group g;
    memset(&g, 0, sizeof g);
    for (int k = 0; k < SDR_RDS_MAX_GROUPS; k++) groups[(size_t)ch * SDR_RDS_MAX_GROUPS + k] = g;
}

__global__ void k_rds_stats(const RdsState* st, sdr_rds_stats* out, int nch) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= nch) return;
    const RdsState& s = st[ch];
    sdr_rds_stats r;
    r.good = s.good, r.corrected = s.ncorrected, r.bad = s.bad, r.slips = s.slips;
    r.acquired = s.acquired, r.lost = s.lost, r.groups = s.groups, r.synced = s.synced;
    out[ch] = r;
}

__global__ void k_rds_soft_stats(const RdsState* st, sdr_rds_soft_stats* out, int nch, int soft_bits) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= nch) return;
    sdr_rds_soft_stats r;
    r.soft_blocks = st[ch].soft_blocks, r.soft_flips = st[ch].soft_flips, r.soft_bits = (uint32_t)soft_bits, r.reserved = 0;
    out[ch] = r;
}

ParityRows parity_rows() {
    ParityRows pr{};
    for (int k = 0; k < 26; k++) {
        const uint32_t sy = sdr_rds_syndrome(1u << k);
        for (int r = 0; r < 10; r++)
            if ((sy >> r) & 1u) pr.r[r] |= 1u << k;
    }
    return pr;
}

}  // namespace
}  // namespace sdrk

using namespace sdrk;

extern "C" {

int sdr_rds_mode_ok(int mode) {
    sdr_info in;
    if (mode < 0 || mode > 3 || mode_info(&in, 1, mode, 1) != SDR_OK) return 0;
    return (long long)in.if_Fs * 247 == 640LL * 2375 * in.symbol_Fs ? 1 : 0;
}

void sdr_rds_soft_opts_default(sdr_rds_soft_opts* o) {
    if (!o) return;
    o->max_burst = 2;
    o->loss_blocks = 8;
    o->soft_bits = 6;
}

// the rules of the options records; `who` names the caller in the text
static int opts_rule(const char* who, int max_burst, int loss_blocks) {
    if (max_burst < 0 || max_burst > 5) return fail(SDR_E_INVALID, "%s: max_burst %d is not in 0..5", who, max_burst);
    if (loss_blocks < 1 || loss_blocks > 64) return fail(SDR_E_INVALID, "%s: loss_blocks %d is not in 1..64", who, loss_blocks);
    return SDR_OK;
}
static int soft_bits_rule(const char* who, int soft_bits) {
    if (soft_bits < 0 || soft_bits > 6) return fail(SDR_E_INVALID, "%s: soft_bits %d is not in 0..6", who, soft_bits);
    return SDR_OK;
}

int sdr_rds_opts_check(const sdr_rds_opts* opts) {
    if (!opts) return fail(SDR_E_INVALID, "rds_opts_check: opts is NULL");
    return opts_rule("rds_opts_check", opts->max_burst, opts->loss_blocks);
}

int sdr_rds_soft_opts_check(const sdr_rds_soft_opts* opts) {
    if (!opts) return fail(SDR_E_INVALID, "rds_soft_opts_check: opts is NULL");
    if (const int r = soft_bits_rule("rds_soft_opts_check", opts->soft_bits)) return r;
    return opts_rule("rds_soft_opts_check", opts->max_burst, opts->loss_blocks);
}

// soft_bits < 0: a handle of sdr_rds_dec_create
static int dec_create(sdr_rds_dec** out, int device, int nch, const sdr_rds_opts* opts, int soft_bits) {
    if (!out) return fail(SDR_E_INVALID, "rds_dec_create: out is NULL");
    *out = nullptr;
    if (!opts) return fail(SDR_E_INVALID, "rds_dec_create: opts is NULL");
    if (nch < 1) return fail(SDR_E_INVALID, "rds_dec_create: nch %d < 1", nch);
    if (const int r = opts_rule("rds_dec_create", opts->max_burst, opts->loss_blocks)) return r;
    uint32_t tab[1024];
    if (sdr_rds_correction_table(opts->max_burst, tab, nullptr) != SDR_OK)
        return fail(SDR_E_INVALID, "rds_dec_create: no correction table");
    sdr_rds_dec* d = nullptr;
    if (const int r = create_begin(&d, device, "rds_dec_create")) return r;
    d->nch = nch;
    d->max_burst = opts->max_burst;
    d->loss_blocks = opts->loss_blocks;
    d->soft = soft_bits >= 0;
    d->soft_bits = soft_bits >= 0 ? soft_bits : 0;
    hipError_t e = hipSuccess;
    dev_alloc(e, &d->st, (size_t)nch * sizeof(RdsState));
    if (d->soft) dev_alloc(e, &d->hist, (size_t)nch * SOFT_HIST * sizeof(uint16_t));
    dev_alloc(e, &d->sstats, (size_t)nch * sizeof(sdr_rds_soft_stats));
    dev_alloc(e, &d->tab, sizeof tab);
    dev_alloc(e, &d->groups, (size_t)nch * SDR_RDS_MAX_GROUPS * sizeof(sdr_rds_group));
    dev_alloc(e, &d->ngroups, (size_t)nch * sizeof(int32_t));
    dev_alloc(e, &d->stats, (size_t)nch * sizeof(sdr_rds_stats));
    if (e == hipSuccess) e = hipMemcpy(d->tab, tab, sizeof tab, hipMemcpyHostToDevice);
    create_reset(e, k_rds_reset, groups256(nch), d->st, d->groups, d->ngroups, nch, d->hist);
    return create_done(e, d, out, sdr_rds_dec_destroy, "rds_dec_create");
}

int sdr_rds_dec_create(sdr_rds_dec** out, int device, int nch, const sdr_rds_opts* opts) {
    return dec_create(out, device, nch, opts, -1);
}

int sdr_rds_dec_create_soft(sdr_rds_dec** out, int device, int nch, const sdr_rds_soft_opts* opts) {
    if (!out) return fail(SDR_E_INVALID, "rds_dec_create_soft: out is NULL");
    *out = nullptr;
    if (!opts) return fail(SDR_E_INVALID, "rds_dec_create_soft: opts is NULL");
    if (const int r = soft_bits_rule("rds_dec_create_soft", opts->soft_bits)) return r;
    const sdr_rds_opts ro{opts->max_burst, opts->loss_blocks};
    return dec_create(out, device, nch, &ro, opts->soft_bits);
}

int sdr_rds_dec_destroy(sdr_rds_dec* d) {
    if (!d) return fail(SDR_E_INVALID, "rds_dec_destroy: null handle");
    return destroy_handle(d, {d->st, d->tab, d->groups, d->ngroups, d->stats, d->hist, d->sstats});
}

int sdr_rds_dec_reset(sdr_rds_dec* d, void* stream) {
    if (!d) return fail(SDR_E_INVALID, "rds_dec_reset: null handle");
    return launch_on(d->device, k_rds_reset, groups256(d->nch), S(stream), d->st, d->groups, d->ngroups, d->nch, d->hist);
}

int sdr_rds_groups(sdr_rds_dec* d, const int32_t* nbits_dev, const uint8_t* bits_dev, size_t bits_stride, void* stream) {
    if (!d || !nbits_dev || !bits_dev) return fail(SDR_E_INVALID, "rds_groups: null argument");
    if (bits_stride < SDR_MAX_BITS)
        return fail(SDR_E_INVALID, "rds_groups: bits_stride %zu < SDR_MAX_BITS = %d", bits_stride, SDR_MAX_BITS);
    if (d->soft) return fail(SDR_E_INVALID, "rds_groups: a handle of sdr_rds_dec_create_soft takes sdr_rds_groups_soft");
    HIP_TRY(hipSetDevice(d->device));
    static const ParityRows pr = parity_rows();
    hipLaunchKernelGGL(k_rds_groups<false>, dim3(d->nch), dim3(64), 0, (hipStream_t)stream, (RdsState*)d->st, nbits_dev,
                       bits_dev, bits_stride, (const uint32_t*)d->tab, d->groups, d->ngroups, d->loss_blocks, pr,
                       (const uint16_t*)nullptr, (size_t)0, (uint16_t*)nullptr, 0);
    LAUNCH_CHECK();
    return SDR_OK;
}

int sdr_rds_groups_soft(sdr_rds_dec* d, const int32_t* nbits_dev, const uint8_t* bits_dev, size_t bits_stride,
                        const uint16_t* soft_dev, size_t soft_stride, void* stream) {
    if (!d || !nbits_dev || !bits_dev || !soft_dev) return fail(SDR_E_INVALID, "rds_groups_soft: null argument");
    if (bits_stride < SDR_MAX_BITS)
        return fail(SDR_E_INVALID, "rds_groups_soft: bits_stride %zu < SDR_MAX_BITS = %d", bits_stride, SDR_MAX_BITS);
    if (soft_stride < SDR_MAX_BITS)
        return fail(SDR_E_INVALID, "rds_groups_soft: soft_stride %zu < SDR_MAX_BITS = %d", soft_stride, SDR_MAX_BITS);
    if (reinterpret_cast<uintptr_t>(soft_dev) & 1) return fail(SDR_E_INVALID, "rds_groups_soft: soft_dev is not a uint16 pointer");
    if (!d->soft) return fail(SDR_E_INVALID, "rds_groups_soft: a handle of sdr_rds_dec_create takes sdr_rds_groups");
    HIP_TRY(hipSetDevice(d->device));
    static const ParityRows pr = parity_rows();
    hipLaunchKernelGGL(k_rds_groups<true>, dim3(d->nch), dim3(64), 0, (hipStream_t)stream, (RdsState*)d->st, nbits_dev,
                       bits_dev, bits_stride, (const uint32_t*)d->tab, d->groups, d->ngroups, d->loss_blocks, pr, soft_dev,
                       soft_stride, d->hist, d->soft_bits);
    LAUNCH_CHECK();
    return SDR_OK;
}

int sdr_rds_groups_copy(sdr_rds_dec* d, sdr_rds_group* host_groups, int32_t* host_ngroups, void* stream) {
    if (!d || !host_groups || !host_ngroups) return fail(SDR_E_INVALID, "rds_groups_copy: null argument");
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipMemcpyAsync(host_groups, d->groups, (size_t)d->nch * SDR_RDS_MAX_GROUPS * sizeof(sdr_rds_group),
                           hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipMemcpyAsync(host_ngroups, d->ngroups, (size_t)d->nch * sizeof(int32_t), hipMemcpyDeviceToHost,
                           (hipStream_t)stream));
    return SDR_OK;
}

int sdr_rds_groups_read(sdr_rds_dec* d, sdr_rds_group* host_groups, int32_t* host_ngroups, void* stream) {
    if (const int r = sdr_rds_groups_copy(d, host_groups, host_ngroups, stream)) return r;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return SDR_OK;
}

int sdr_rds_stats_read(sdr_rds_dec* d, sdr_rds_stats* host_stats, void* stream) {
    if (!d || !host_stats) return fail(SDR_E_INVALID, "rds_stats_read: null argument");
    if (const int r = launch_on(d->device, k_rds_stats, groups256(d->nch), S(stream), d->st, d->stats, d->nch)) return r;
    return copy_records(d->stats, host_stats, d->nch, S(stream));
}

int sdr_rds_soft_stats_read(sdr_rds_dec* d, sdr_rds_soft_stats* host_stats, void* stream) {
    if (!d || !host_stats) return fail(SDR_E_INVALID, "rds_soft_stats_read: null argument");
    if (const int r = launch_on(d->device, k_rds_soft_stats, groups256(d->nch), S(stream), d->st, d->sstats, d->nch, d->soft_bits))
        return r;
    return copy_records(d->sstats, host_stats, d->nch, S(stream));
}

}  // extern "C"
