// sdr_plls.cpp -- host protocol of the persistent PLL launch (no kernels): one launch of
// k_pll_multi (sdr_pll.hip launch_pll_multi) runs the PLLs of many blocks; the host prepares its
// device words and stamp arrays, launches it on a CU-masked stream, signals each block's input,
// waits for each block's phases on the post streams and reports the launch's times. It owns
// sdr_ctx::pers: the sequence numbers of the blocks launched, signalled and waited for.

#include "sdr_internal.h"

#include <algorithm>
#include <vector>

using namespace sdrk;

namespace {

// the bookkeeping of a persistent launch: recover an abandoned previous launch, allocate the words
// and stamp arrays, reset this launch's stamps and error word (stream order on `stream`)
int plls_prepare(sdr_ctx* c, int nblocks, hipStream_t s) {
    sdr_ctx::Pers& P = c->pers;
    int dev_unused = 0;
    if (P.signaled != P.launched) {
        // blocks of the previous launch were never signalled: its waves give up on them after the
        // bounded wait (PLL_WAIT_TICKS) and still count them done. Let it drain, then resynchronise
        // the host's sequence numbers with the device words so this launch starts clean.
        HIP_TRY(hipStreamSynchronize(P.stream));
        P.signaled = P.waited = P.launched;
        HIP_TRY(hipMemcpyAsync(P.words, &P.launched, sizeof(uint32_t), hipMemcpyHostToDevice, s));
    } else if (P.stream && P.stream != s && P.launched != 0 && masked_stream(P.stream, &dev_unused, nullptr)) {
        // every block of the previous launch is signalled, but its waves may still be stamping its
        // last blocks or setting its error word: the resets below wait for that launch in `s`'s order
        // (a PLL stream destroyed since has completed its work: hipStreamDestroy waits for it)
        if (!P.ev) HIP_TRY(hipEventCreateWithFlags(&P.ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(P.ev, P.stream));
        HIP_TRY(hipStreamWaitEvent(s, P.ev, 0));
    }
    if (!P.words) {
        void* w = nullptr;
        HIP_TRY(hipMalloc(&w, PLL_WORDS * sizeof(uint32_t)));
        c->allocs.push_back(w);
        P.words = static_cast<uint32_t*>(w);
        HIP_TRY(hipMemsetAsync(P.words, 0, PLL_WORDS * sizeof(uint32_t), s));
    }
    if (P.tcap < nblocks) {
        // timestamp arrays: allocated once with room for long phases (a later, longer launch
        // grows them here, outside any timed loop that reuses the capacity)
        const int cap = std::max(nblocks, 4096);
        if (P.tcap > 0) HIP_TRY(hipStreamSynchronize(P.stream));   // the last launch still writes them
        void *a = nullptr, *b = nullptr, *cy = nullptr;
        HIP_TRY(hipMalloc(&a, (size_t)cap * sizeof(unsigned long long)));
        c->allocs.push_back(a);
        HIP_TRY(hipMalloc(&b, (size_t)cap * sizeof(unsigned long long)));
        c->allocs.push_back(b);
        HIP_TRY(hipMalloc(&cy, (size_t)cap * 2 * sizeof(unsigned long long)));
        c->allocs.push_back(cy);
        P.t0 = static_cast<unsigned long long*>(a);
        P.t1 = static_cast<unsigned long long*>(b);
        P.cyc = static_cast<unsigned long long*>(cy);
        P.tcap = cap;
    }
    HIP_TRY(hipMemsetAsync(P.t0, 0xFF, (size_t)nblocks * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(P.t1, 0, (size_t)nblocks * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(P.cyc, 0, (size_t)nblocks * 2 * sizeof(unsigned long long), s));
    // err of this launch: cleared after every post stream that read the previous launch's (their
    // queued stages would otherwise poison by a word that no longer says so, or read a clear word for a
    // block the old launch never computed)
    if (P.nreaders > sdr_ctx::Pers::READERS) {
        HIP_TRY(hipDeviceSynchronize());
    } else {
        for (int i = 0; i < P.nreaders; i++)   // recorded by the readers (pers_reader_mark)
            if (P.reader_ev[i]) HIP_TRY(hipStreamWaitEvent(s, P.reader_ev[i], 0));
    }
    P.nreaders = 0;
    HIP_TRY(hipMemsetAsync(P.words + 1, 0, sizeof(uint32_t), s));
    P.prepared = nblocks;
    P.prepared_launch = P.launched;
    return SDR_OK;
}

// the persistent launch's jobs: the selected PLLs (SDR_PLLS_STEREO, SDR_PLLS_RDS; in that order in
// j[]) of the two parities, p[0] = the parity the next sdr_frontend switches to
PllJobs2 plls_jobs(sdr_ctx* c, int which, int* njobs) {
    PllJobs2 jobs{};
    const int first_parity = c->parity ^ 1;
    for (int k = 0; k < 2; k++) {
        const int saved = c->parity;
        c->parity = first_parity ^ k;
        int q = 0;
        if (which & SDR_PLLS_STEREO) jobs.p[k].j[q++] = stereo_job(c);
        if (which & SDR_PLLS_RDS) jobs.p[k].j[q++] = rds_job(c);
        *njobs = q;
        c->parity = saved;
    }
    return jobs;
}

int plls_which_ok(const sdr_ctx* c, int which, const char* what) {
    if (which != SDR_PLLS_STEREO && which != SDR_PLLS_RDS && which != SDR_PLLS_BOTH)
        return fail(SDR_E_INVALID, "%s: which = %d (SDR_PLLS_STEREO, SDR_PLLS_RDS or SDR_PLLS_BOTH)", what, which);
    if ((which & SDR_PLLS_RDS) && !c->rds_on) return fail(SDR_E_INVALID, "%s: the RDS PLL needs rds_on", what);
    return SDR_OK;
}

// the plan of a persistent launch of `which` on a stream over CUs [first_cu, first_cu + n_cu)
int plls_plan_on(sdr_ctx* c, int which, int first_cu, int n_cu, const char* what, PllMultiPlan* P) {
    if (const int r = plls_which_ok(c, which, what)) return r;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    const int ncu = prop.multiProcessorCount;
    if (first_cu < 0 || n_cu <= 0 || first_cu + n_cu > ncu)
        return fail(SDR_E_INVALID, "%s: CUs [%d, %d) outside [0, %d)", what, first_cu, first_cu + n_cu, ncu);
    int nset = 0;
    const std::vector<uint32_t> mask = cu_range_mask(ncu, first_cu, n_cu, 0, &nset);
    const CuPlacement pl = cu_placement(mask.data(), (int)mask.size(), ncu, device_xccs(c->device));
    HIP_TRY(hipSetDevice(c->device));
    int njobs = 0;
    const PllJobs2 jobs = plls_jobs(c, which, &njobs);
    return pll_multi_plan(jobs, njobs, c->info.block_if, c->nch, pl, P);
}

// may `block` be signalled next to the pending persistent launch?
int plls_signal_check(const sdr_ctx* c, long long block, const char* what) {
    const sdr_ctx::Pers& P = c->pers;
    if (P.signaled == P.launched)
        return fail(SDR_E_INVALID, "%s: no sdr_plls_launch covers this block", what);
    // the launch fixed block j's buffer parity as (first block's parity) ^ j: only the blocks that
    // follow the launch, in order, may be signalled
    const long long want_block = P.first_block + (long long)(P.signaled - P.base);
    if (block != want_block)
        return fail(SDR_E_INVALID, "%s: block %lld, but the launch expects block %lld next", what, block, want_block);
    // a block's done slot is reused PLL_DONE_RING sequence numbers later: every block must have been
    // waited for (sdr_plls_wait) before the one that reuses its slot is signalled
    if (P.signaled - P.waited >= PLL_DONE_RING)
        return fail(SDR_E_INVALID, "%s: %u blocks signalled but not waited for (at most %u in flight)", what,
                    P.signaled - P.waited, PLL_DONE_RING);
    return SDR_OK;
}

}  // namespace

namespace sdrk {

int check_pers_failed(const sdr_ctx* c, const char* what) {
    if (c->pers.failed && c->pers.err(c->block))
        return fail(SDR_E_HIP, "%s: the persistent PLL launch of this block timed out (outputs invalid): "
                               "sdr_ctx_reset, then a new sdr_plls_launch", what);
    return SDR_OK;
}

// After a stage that read the persistent launch's error word was enqueued on `s`: record that
// stream's reader event now, so the next launch's prepare can order its reset of the word after
// every reader by waiting on the events alone -- no stream handle is used after the call that
// supplied it (the handle only names the event's slot; a stream destroyed since is never touched).
// More than Pers::READERS streams fall back to a device synchronisation in the prepare.
int pers_reader_mark(sdr_ctx* c, hipStream_t s) {
    sdr_ctx::Pers& P = c->pers;
    if (!P.err(c->block)) return SDR_OK;
    int slot = -1;
    for (int i = 0; i < P.nreaders && i < sdr_ctx::Pers::READERS; i++)
        if (P.readers[i] == s) slot = i;
    if (slot < 0) {
        if (P.nreaders >= sdr_ctx::Pers::READERS) {
            P.nreaders = sdr_ctx::Pers::READERS + 1;
            return SDR_OK;
        }
        slot = P.nreaders++;
        P.readers[slot] = s;
    }
    if (!P.reader_ev[slot]) HIP_TRY(hipEventCreateWithFlags(&P.reader_ev[slot], hipEventDisableTiming));
    HIP_TRY(hipEventRecord(P.reader_ev[slot], s));
    return SDR_OK;
}

int plls_parts_check(const sdr_ctx* c, const char* what) {
    if (c->pers.signaled != c->pers.base)
        return fail(SDR_E_INVALID, "%s: only the first block of a persistent launch comes in parts", what);
    if (c->pers.which != SDR_PLLS_BOTH)
        return fail(SDR_E_INVALID, "%s: the launch must cover both PLLs (sdr_plls_launch)", what);
    return plls_signal_check(c, c->block + 1, what);
}

// (capped below PLL_SUB_SCALE: a count above it would reach the values of a later launch)
int plls_parts_publish(sdr_ctx* c, int tiles, hipStream_t s) {
    return launch_flag_store(c->pers.words + PLL_WORD_SUB,
                             c->pers.base * PLL_SUB_SCALE + std::min((uint32_t)tiles, PLL_SUB_SCALE - 1u), s);
}

}  // namespace sdrk

extern "C" {

int sdr_plls_prepare(sdr_ctx* c, int nblocks, void* stream) {
    if (!c || nblocks <= 0) return fail(SDR_E_INVALID, "plls_prepare: bad arguments");
    if (c->flags & SDR_FLAG_PLL_LIBM) return fail(SDR_E_INVALID, "plls_prepare: not with SDR_FLAG_PLL_LIBM");
    HIP_TRY(hipSetDevice(c->device));
    return plls_prepare(c, nblocks, S(stream));
}

int sdr_plls_fits(sdr_ctx* c, int which, int first_cu, int n_cu, int* waves, long long* groups, long long* resident) {
    if (!c || !waves || !groups || !resident) return fail(SDR_E_INVALID, "plls_fits: bad arguments");
    PllMultiPlan P;
    if (const int r = plls_plan_on(c, which, first_cu, n_cu, "plls_fits", &P)) return r;
    *waves = (int)P.waves;
    *groups = P.groups;
    *resident = P.resident;
    return SDR_OK;
}

// Diagnosis (not part of sdr_amd.h): which kernel sdr_plls_launch_sel(which) takes on a stream over CUs
// [first_cu, first_cu + n_cu). out = [waves per workgroup, 1: the LDS-staged loop (pll_run_split_coal),
// 1: the trigArg table fits LDS (TAB = true until w * trigOffset passes PLL_TAB_WT_MAX), dynamic LDS
// bytes]. Nothing is enqueued.
int sdr_diag_plls_plan(sdr_ctx* c, int which, int first_cu, int n_cu, int out[4]) {
    if (!c || !out) return fail(SDR_E_INVALID, "diag_plls_plan: bad arguments");
    PllMultiPlan P;
    if (const int r = plls_plan_on(c, which, first_cu, n_cu, "diag_plls_plan", &P)) return r;
    out[0] = P.WG;
    out[1] = P.staged;
    out[2] = P.tab_ok;
    out[3] = (int)P.lds;
    return SDR_OK;
}

int sdr_plls_launch(sdr_ctx* c, int nblocks, void* stream) { return sdr_plls_launch_sel(c, nblocks, SDR_PLLS_BOTH, stream); }

int sdr_plls_launch_sel(sdr_ctx* c, int nblocks, int which, void* stream) {
    if (!c || nblocks <= 0) return fail(SDR_E_INVALID, "plls_launch: bad arguments");
    if (const int rf_ = check_failed(c, "plls_launch")) return rf_;
    if (c->flags & SDR_FLAG_PLL_LIBM) return fail(SDR_E_INVALID, "plls_launch: not with SDR_FLAG_PLL_LIBM");
    if (const int r = plls_which_ok(c, which, "plls_launch")) return r;
    hipStream_t s = S(stream);
    // the launch's waves spin until later dispatches on other streams publish each block, so the
    // PLL stream must own its hardware queue (pool streams share GPU_MAX_HW_QUEUES queues with the
    // streams that signal) and every workgroup must be resident on the stream's CUs at once: refused
    // before anything is enqueued otherwise (a waiting launch could never finish, and its blocks would
    // time out)
    int sdev = -1;
    CuPlacement pl;
    if (!masked_stream(s, &sdev, &pl))
        return fail(SDR_E_INVALID, "plls_launch: the PLL stream was not made by sdr_stream_create_cu_range (a "
                                   "persistent launch needs a stream with its own hardware queue; use sdr_plls)");
    if (sdev != c->device)
        return fail(SDR_E_INVALID, "plls_launch: the PLL stream is on device %d, the context on %d", sdev, c->device);
    HIP_TRY(hipSetDevice(c->device));
    const int n = c->info.block_if, nch = c->nch;
    int njobs = 0;
    const PllJobs2 jobs = plls_jobs(c, which, &njobs);
    {
        PllMultiPlan P;
        if (const int r = pll_multi_plan(jobs, njobs, n, nch, pl, &P)) return r;
        if (P.groups > P.resident)
            return fail(SDR_E_INVALID, "plls_launch: %u waves do not fit the stream's %d CUs: %lld of %lld workgroups "
                        "of %d waves resident at once (%d per CU, %d XCCs x %d SE-balanced CU slots; use sdr_plls, "
                        "a stream over more CUs, or sdr_plls_fits to pick one)", P.waves, pl.ncu, P.resident,
                        P.groups, P.WG, P.per_cu, pl.xcc_active, pl.min_units);
    }
    sdr_ctx::Pers& P = c->pers;
    // prepared ahead (sdr_plls_prepare, same nblocks, no launch since): only the launch is left
    if (!(P.prepared == nblocks && P.prepared_launch == P.launched && P.signaled == P.launched)) {
        const int r = plls_prepare(c, nblocks, s);
        if (r) return r;
    }
    P.prepared = 0;
    uint32_t waves = 0;
    const int r = launch_pll_multi(jobs, njobs, n, nch, nblocks, P.words, P.launched, P.t0, P.t1, P.cyc, &waves, s, pl,
                                   FRB_TILE);
    if (r) return r;
    P.which = which;
    P.failed = false;   // this launch's error word was cleared by its prepare
    P.waves = waves;
    P.base = P.launched;
    P.first_block = c->block + 1;       // the block the next sdr_frontend produces
    P.stream = s;
    P.launched += (uint32_t)nblocks;
    P.last_n = nblocks;
    return SDR_OK;
}

int sdr_plls_signal(sdr_ctx* c, void* stream) {
    if (!c) return fail(SDR_E_INVALID, "null context");
    if (const int rf_ = check_failed(c, "plls_signal")) return rf_;
    sdr_ctx::Pers& P = c->pers;
    const bool st = (P.which & SDR_PLLS_STEREO) != 0, rd = (P.which & SDR_PLLS_RDS) != 0;
    if ((st && (c->st_pre_done != c->block || c->st_pll_done == c->block)) ||
        (rd && (c->rds_pre_done != c->block || c->rds_pll_done == c->block)))
        return fail(SDR_E_INVALID, "plls_signal: run the pre part of every PLL the launch covers (sdr_stereo_pre, "
                                   "sdr_rds_pre) on a new block first");
    if (const int rc = plls_signal_check(c, c->block, "plls_signal")) return rc;
    const int r = launch_flag_store(P.words, P.signaled + 1u, S(stream));
    if (r) return r;
    P.block = c->block;
    P.block_seq = P.signaled;
    P.signaled++;
    if (st) c->st_pll_done = c->block;
    if (rd) c->rds_pll_done = c->block;
    return SDR_OK;
}

int sdr_plls_wait(sdr_ctx* c, void* stream) {
    if (!c) return fail(SDR_E_INVALID, "null context");
    if (const int rf_ = check_failed(c, "plls_wait")) return rf_;
    sdr_ctx::Pers& P = c->pers;
    if (P.block != c->block) return fail(SDR_E_INVALID, "plls_wait: sdr_plls_signal this block first");
    // every wave has finished this block's sequence number (its slot of the done ring)
    const uint32_t seq = P.block_seq;
    const uint32_t want = P.waves * (seq / PLL_DONE_RING + 1u);
    if ((int32_t)(seq + 1u - P.waited) > 0) P.waited = seq + 1u;
    // this stream's post stages read the launch's error word: the next prepare orders its reset after
    // them (a post stream not in the list -- more than Pers::READERS of them -- falls back to a device
    // synchronisation there)
    hipStream_t ws = S(stream);
    if (const int r = launch_flag_wait(P.words + PLL_WORDS_DONE + seq % PLL_DONE_RING, want, P.words + 1, ws))
        return r;
    return pers_reader_mark(c, ws);
}

int sdr_plls_report(sdr_ctx* c, double* block_ms, int max_blocks, int* nblocks, void* stream) {
    if (!c || !c->pers.words) return fail(SDR_E_INVALID, "plls_report: no persistent launch");
    sdr_ctx::Pers& P = c->pers;
    hipStream_t s = S(stream);
    const int n = std::min(P.last_n, std::max(max_blocks, 0));
    std::vector<unsigned long long> t0((size_t)std::max(n, 1)), t1((size_t)std::max(n, 1));
    uint32_t words[PLL_WORDS] = {};
    HIP_TRY(hipMemcpyAsync(words, P.words, sizeof(words), hipMemcpyDeviceToHost, s));
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(t0.data(), P.t0, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(t1.data(), P.t1, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    // block j's PLL time: from when both its input was signalled and the previous block was done
    // (waves drift apart, so the first wave's start can precede the slowest wave's previous end)
    // to its last wave's end, from the 100 MHz s_memrealtime stamps
    for (int j = 0; j < n && block_ms; j++) {
        const unsigned long long from = j > 0 ? std::max(t0[j], t1[j - 1]) : t0[j];
        block_ms[j] = (t1[j] >= from) ? (double)(t1[j] - from) * 1e-5 : -1.0;
    }
    if (nblocks) *nblocks = n;
    if (words[1]) {
        P.failed = true;
        return fail(SDR_E_HIP, "plls_report: a persistent PLL wait timed out (outputs invalid): err %u, flag %u, "
                    "signalled %u, launched %u, waves %u", words[1], words[0], P.signaled, P.launched, P.waves);
    }
    return SDR_OK;
}

int sdr_plls_timeline(sdr_ctx* c, unsigned long long* t_start, unsigned long long* t_end, int max_blocks, int* nblocks,
                      void* stream) {
    if (!c || !c->pers.words) return fail(SDR_E_INVALID, "plls_timeline: no persistent launch");
    hipStream_t s = S(stream);
    const int n = std::min(c->pers.last_n, std::max(max_blocks, 0));
    if (n > 0 && t_start)
        HIP_TRY(hipMemcpyAsync(t_start, c->pers.t0, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (n > 0 && t_end)
        HIP_TRY(hipMemcpyAsync(t_end, c->pers.t1, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (nblocks) *nblocks = n;
    return SDR_OK;
}

int sdr_plls_cycles(sdr_ctx* c, double* cycles_per_step, double* clock_mhz, void* stream) {
    if (!c || !c->pers.cyc || c->pers.last_n <= 0) return fail(SDR_E_INVALID, "plls_cycles: no persistent launch");
    hipStream_t s = S(stream);
    const int n = c->pers.last_n;
    std::vector<unsigned long long> v((size_t)2 * n);
    HIP_TRY(hipMemcpyAsync(v.data(), c->pers.cyc, v.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    double cyc = 0.0, ticks = 0.0;
    for (int j = 0; j < n; j++) {
        cyc += (double)v[2 * j];
        ticks += (double)v[2 * j + 1];
    }
    const double steps = (double)c->pers.waves * n * c->info.block_if;
    if (cycles_per_step) *cycles_per_step = steps > 0 ? cyc / steps : -1.0;
    if (clock_mhz) *clock_mhz = ticks > 0 ? cyc / ticks * 100.0 : -1.0;   // s_memrealtime runs at 100 MHz
    return SDR_OK;
}

int sdr_plls_block_cycles(sdr_ctx* c, double* cycles_per_step, double* clock_mhz, int max, int* n_out, void* stream) {
    if (!c || !c->pers.cyc || c->pers.last_n <= 0) return fail(SDR_E_INVALID, "plls_block_cycles: no persistent launch");
    hipStream_t s = S(stream);
    const int n = c->pers.last_n;
    std::vector<unsigned long long> v((size_t)2 * n);
    HIP_TRY(hipMemcpyAsync(v.data(), c->pers.cyc, v.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const double steps = (double)c->pers.waves * c->info.block_if;
    for (int j = 0; j < n && j < max; j++) {
        if (cycles_per_step) cycles_per_step[j] = steps > 0 ? (double)v[2 * j] / steps : -1.0;
        if (clock_mhz) clock_mhz[j] = v[2 * j + 1] ? (double)v[2 * j] / (double)v[2 * j + 1] * 100.0 : -1.0;
    }
    if (n_out) *n_out = n;
    return SDR_OK;
}

}  // extern "C"
