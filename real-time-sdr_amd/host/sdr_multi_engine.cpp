// sdr_multi_engine.cpp -- the multi-channel receiver engine (include/sdr_multi.h): the reference
// program's three stage threads (project.cpp:134-136: RF front end, audio, RDS) over nch channels at
// once, on the C ABI of libsdr_amd.so, joined by the reference's queue protocol with the payload on
// the device (include/dropin/fm_batch.h). The CLI real-time-sdr_amd/bin/sdr_multi (sdr_multi.cpp) and
// bench.py's queue_plumbed leg run it.
//
// Threads (per block b; every device hand-off is a HIP event or a device flag, no thread waits for
// another's GPU work except through the queue's prepare() ordering):
//   reader  file/stdin -> pinned ring slot (byte-stream input only)
//   RF      [slot -H2D (copy stream)-> d_iq] or the device-resident block; sdr_frontend (a tuned run,
//           include/sdr_multi_tuned.h: sdr_frontend_tuned on nsrc capture rows per block; a wide run,
//           include/sdr_multi_wide.h: sdr_split_block of the wide block into one of two row buffers
//           first, on the same stream, and sdr_frontend_tuned on that buffer); fm_demod ->
//           a recycled FmBatch (device), event, push                     rffrontend.cpp:45-76
//   audio   wait_and_pop(0); sdr_push_fm_demod; stereo_pre; PLL; stereo_post; L/R -D2H-> pinned;
//           the write of block b-1 overlaps the GPU work of block b          stereo.cpp:69-114
//   rds     wait_and_pop(1); sdr_push_fm_demod; rds_pre; PLL; rds_post; rds_bits -D2H-> host;
//           frame sync per channel every 15 decoding blocks (host)          rds.cpp:95-192
// A metered run (include/sdr_multi_meter.h) adds sdr_meter_audio after the audio thread's stereo_post
// and sdr_meter_rds after the RDS thread's rds_post, each on its own context and post stream, both on
// one shared meter; each thread copies the rows out behind its call and hands its part of block b to
// MeterOut, which joins the two parts, writes PREFIX.meter and keeps the run's sums for PREFIX.status.
// A finished run (include/sdr_multi_audio.h) adds, behind them on the audio thread's post stream,
// sdr_audio_blend_from_meter (with --blend) and sdr_audio_finish from the block's L/R rows into rows of
// its own, copied out behind the L/R copy and written to PREFIX.audio.
// Streams (the four-queue budget of DESIGN.md 5): the producer's front end and both consumers' pre
// parts share one stream (s_fe), both consumers' post parts another (s_post), and each consumer's
// PLL has its own CU-masked stream -- with a known block count ONE persistent launch per consumer
// (sdr_plls_launch_sel: the stereo PLL on CUs [0, pll_cus/2), the RDS PLL on [pll_cus/2, pll_cus)),
// signalled from s_fe and waited for on s_post; otherwise one dispatch per block. s_fe and s_post
// run on the CUs the PLLs leave. A consumer's wait on s_post is enqueued after its signal on s_fe
// and its next parity reuse on s_fe after its post on s_post, so no wait on one stream can sit in
// front of the work it waits for on the other.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>

#include <sys/stat.h>
#include <unistd.h>
#include <vector>

#include "fm_batch.h"
#include "hip_util.h"
#include "rds_utilities.h"
#include "sdr_amd.h"
#include "sdr_multi.h"
#include "sdr_multi_audio.h"
#include "sdr_multi_meter.h"
#include "sdr_multi_tuned.h"
#include "sdr_multi_wide.h"

using sdrhost::check_hip;
using sdrhost::check_sdr;
using sdrhost::die;

namespace {

hipStream_t plain_stream() {
    hipStream_t h = nullptr;
    check_hip(hipStreamCreateWithFlags(&h, hipStreamNonBlocking), "hipStreamCreate");
    return h;
}

// a stream on CUs [first, first + n) (exclude = 0) or on every other CU (exclude = 1); its own
// hardware queue (sdr_stream_create_cu_range). Streams outlive a run, like the pinned buffers below:
// making and destroying the six masked streams took ~30 + ~40 ms per run, in which the GPU idled
// and its clock fell before the next run's first blocks (profiles/r06/queue_fill/). A run takes idle
// pooled streams of its CU range; SDR_MULTI_STREAM_CACHE=0: made and destroyed per run.
struct PooledStream {
    int device, first, n, exclude;
    void* s;
};
std::mutex g_stream_mu;
std::vector<PooledStream> g_stream_free, g_stream_live;
bool stream_cache_on() {
    const char* e = std::getenv("SDR_MULTI_STREAM_CACHE");
    return !e || std::atoi(e) != 0;
}
hipStream_t masked_stream(int device, int first, int n, int exclude) {
    std::lock_guard<std::mutex> lk(g_stream_mu);
    for (size_t i = 0; i < g_stream_free.size(); i++) {
        const PooledStream& p = g_stream_free[i];
        if (p.device == device && p.first == first && p.n == n && p.exclude == exclude) {
            g_stream_live.push_back(p);
            g_stream_free.erase(g_stream_free.begin() + (long)i);
            return (hipStream_t)g_stream_live.back().s;
        }
    }
    void* s = nullptr;
    check_sdr(sdr_stream_create_cu_range(&s, device, first, n, exclude), "sdr_stream_create_cu_range");
    g_stream_live.push_back({device, first, n, exclude, s});
    return (hipStream_t)s;
}
// the end of a run: the stream (idle by then) back to the pool, or destroyed
void release_masked(hipStream_t h) {
    std::lock_guard<std::mutex> lk(g_stream_mu);
    for (size_t i = 0; i < g_stream_live.size(); i++)
        if (g_stream_live[i].s == (void*)h) {
            if (stream_cache_on()) g_stream_free.push_back(g_stream_live[i]);
            else (void)sdr_stream_destroy(h);
            g_stream_live.erase(g_stream_live.begin() + (long)i);
            return;
        }
}

// contexts outlive a run too (SDR_MULTI_CTX_CACHE=0: made and destroyed per run): a later run with
// the same channels, mode and flags takes an idle one back to the reference's initial state
// (sdr_ctx_reset) in ~1 ms instead of ~3 ms to make and ~10 ms to destroy, with the GPU idle meanwhile
struct PooledCtx {
    int device, nch, mode, rds_on, flags;
    sdr_ctx* c;
};
std::mutex g_ctx_mu;
std::vector<PooledCtx> g_ctx_free;
std::vector<PooledCtx> g_ctx_live;
bool ctx_cache_on() {
    const char* e = std::getenv("SDR_MULTI_CTX_CACHE");
    return !e || std::atoi(e) != 0;
}
sdr_ctx* ctx_get(int device, int nch, int mode, int rds_on, int flags) {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    for (size_t i = 0; i < g_ctx_free.size(); i++) {
        const PooledCtx& p = g_ctx_free[i];
        if (p.device == device && p.nch == nch && p.mode == mode && p.rds_on == rds_on && p.flags == flags) {
            check_sdr(sdr_ctx_reset(p.c, nullptr), "sdr_ctx_reset");
            g_ctx_live.push_back(p);
            g_ctx_free.erase(g_ctx_free.begin() + (long)i);
            return g_ctx_live.back().c;
        }
    }
    sdr_ctx* c = nullptr;
    check_sdr(sdr_ctx_create(&c, device, nch, mode, rds_on, flags), "sdr_ctx_create");
    g_ctx_live.push_back({device, nch, mode, rds_on, flags, c});
    return c;
}
void ctx_put(sdr_ctx* c) {   // after the run's streams have drained
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    for (size_t i = 0; i < g_ctx_live.size(); i++)
        if (g_ctx_live[i].c == c) {
            if (ctx_cache_on()) g_ctx_free.push_back(g_ctx_live[i]);
            else sdr_ctx_destroy(c);
            g_ctx_live.erase(g_ctx_live.begin() + (long)i);
            return;
        }
    sdr_ctx_destroy(c);
}

hipEvent_t new_event() {
    hipEvent_t e = nullptr;
    check_hip(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    return e;
}

// ------------------------------------------------------------------ reader: input -> pinned ring
struct Reader {
    static constexpr int SLOTS = 4;   // pinned input slots: the read of block b+2..b+3 rides out host jitter
    FILE* f = nullptr;
    size_t bytes = 0;
    uint8_t* slot[SLOTS] = {};
    hipEvent_t consumed[SLOTS] = {};    // the H2D copy out of the slot has completed
    bool armed[SLOTS] = {};
    std::mutex m;
    std::condition_variable cv;
    std::deque<int> filled, empty;
    bool eof = false;
    double read_s = 0.0;                // time spent reading (the input side of the I/O)
    int readers = 8;                    // pread threads per block (regular files; SDR_MULTI_READERS)
    long long file_size = 0, offset = 0;
    std::thread th;

    Reader(const std::string& path, size_t block_bytes) : bytes(block_bytes) {
        f = path == "-" ? stdin : std::fopen(path.c_str(), "rb");
        if (!f) die("cannot open " + path);
        if (f != stdin) {   // a regular file is read by several threads at once (pread of a block's parts)
            struct stat sb;
            if (fstat(fileno(f), &sb) == 0 && S_ISREG(sb.st_mode)) {
                file_size = (long long)sb.st_size;
                if (const char* e = std::getenv("SDR_MULTI_READERS")) readers = std::max(1, std::atoi(e));
            } else {
                readers = 1;
            }
        } else {
            readers = 1;
        }
        for (int i = 0; i < SLOTS; i++) {
            check_hip(hipHostMalloc(reinterpret_cast<void**>(&slot[i]), bytes, hipHostMallocDefault), "hipHostMalloc");
            consumed[i] = new_event();
            empty.push_back(i);
        }
        th = std::thread([this] { run(); });
    }
    void run() {
        for (;;) {
            int i;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [this] { return !empty.empty(); });
                i = empty.front();
                empty.pop_front();
            }
            if (armed[i]) check_hip(hipEventSynchronize(consumed[i]), "hipEventSynchronize");
            const auto r0 = std::chrono::steady_clock::now();
            const size_t got = readers > 1 ? pread_block(slot[i]) : std::fread(slot[i], 1, bytes, f);
            read_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - r0).count();
            std::lock_guard<std::mutex> lk(m);
            if (got < bytes) {             // a partial block ends the stream (rffrontend.cpp:50-52)
                eof = true;
                cv.notify_all();
                return;
            }
            filled.push_back(i);
            cv.notify_all();
        }
    }
    // one block by `readers` threads, each a contiguous part (pread at the block's file offset)
    size_t pread_block(uint8_t* dst) {
        if (offset + (long long)bytes > file_size) return 0;   // a partial block ends the stream
        const size_t part = (bytes / readers + 4095) / 4096 * 4096;
        std::vector<std::thread> th_;
        std::vector<size_t> got_(readers, 0);
        for (int r = 0; r < readers; r++) {
            const size_t lo = std::min(bytes, part * r), hi = std::min(bytes, part * (r + 1));
            th_.emplace_back([&, r, lo, hi] {
                size_t done = 0;
                while (lo + done < hi) {
                    const ssize_t k = ::pread(fileno(f), dst + lo + done, hi - lo - done, offset + (long long)(lo + done));
                    if (k <= 0) break;
                    done += (size_t)k;
                }
                got_[r] = done;
            });
        }
        size_t got = 0;
        for (int r = 0; r < readers; r++) {
            th_[r].join();
            got += got_[r];
        }
        offset += (long long)got;
        return got;
    }
    int next() {   // a filled slot, or -1 at the end of the input
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [this] { return !filled.empty() || eof; });
        if (filled.empty()) return -1;
        const int i = filled.front();
        filled.pop_front();
        return i;
    }
    void release(int i, hipStream_t copy_stream) {   // after the H2D copy of slot i is enqueued
        check_hip(hipEventRecord(consumed[i], copy_stream), "hipEventRecord");
        std::lock_guard<std::mutex> lk(m);
        armed[i] = true;
        empty.push_back(i);
        cv.notify_all();
    }
    ~Reader() {
        if (th.joinable()) th.join();
        for (int i = 0; i < SLOTS; i++) (void)hipHostFree(slot[i]);
        if (f && f != stdin) std::fclose(f);
    }
};

// per-consumer device/pinned buffers and events, made before the clock starts
// The host handles block b's outputs (PCM write, RDS frame layer, captures) after enqueuing block
// b + LAG's work, so its wait for b's copies never delays the next blocks' signals to the PLLs
// (LAG 1 measured 0.70-0.81 ms per block against 0.687 for the same GPU work in one thread, bench.py)
constexpr int LAG = 2, NH = LAG + 1;   // pinned output buffers in rotation
struct AudioRes {
    hipEvent_t pre = nullptr, pll = nullptr, post = nullptr, out_ready[NH] = {}, d0[NH] = {}, d1[NH] = {};
    int16_t *d_lr[2] = {}, *h_lr[NH] = {};
};
struct RdsRes {
    hipEvent_t pre = nullptr, pll = nullptr, out_ready[NH] = {};
    int32_t *d_nbits = nullptr, *h_nbits[NH] = {};
    uint8_t *d_bits = nullptr, *h_bits[NH] = {};
};

// A metered run's host side. Each consumer copies the meter's rows out after its own call and takes
// from the copy only the fields that call wrote (the other consumer may be writing its own meanwhile);
// the block's row is complete, and written, when both parts are in. The consumers stay within a few
// blocks of each other (the queue's prepare()), so few parts ever wait.
struct MeterOut {
    sdr_meter* m = nullptr;
    sdr_meter_opts mo{};
    int nch = 0, mode = 0;
    uint8_t* h_rows[2][LAG + 1] = {};    // pinned, per consumer and rotation slot: nch rows
    FILE* f = nullptr;                   // PREFIX.meter
    std::mutex mu;
    std::deque<std::pair<long long, std::vector<sdr_meter_row>>> pending[2];
    long long blocks = 0;
    struct Sum {
        double v[5] = {};                // offset, level_db, pilot_nr, rds_nr, eye_db
        long long flag[4] = {};          // blocks with STEREO, RDS, OFFTUNE, DEAD_AIR
    };
    std::vector<Sum> sum;
    // consumer `which` (0 audio, 1 RDS) hands in its copy of block blk's rows
    void part(long long blk, int which, const uint8_t* rows) {
        std::vector<sdr_meter_row> mine((size_t)nch);
        std::memcpy(mine.data(), rows, (size_t)nch * sizeof(sdr_meter_row));
        std::lock_guard<std::mutex> lk(mu);
        auto& other = pending[which ^ 1];
        if (other.empty() || other.front().first != blk) {   // (both hand their blocks in ascending order)
            pending[which].emplace_back(blk, std::move(mine));
            return;
        }
        const std::vector<sdr_meter_row>& a = which == 0 ? mine : other.front().second;
        const std::vector<sdr_meter_row>& r = which == 0 ? other.front().second : mine;
        std::vector<sdr_meter_row> out(a);
        for (int c = 0; c < nch; c++) {
            sdr_meter_row& o = out[(size_t)c];
            const sdr_meter_row& q = r[(size_t)c];
            o.rds_sq = q.rds_sq;
            o.eye_abs = q.eye_abs;
            o.eye_sq = q.eye_sq;
            o.eye_n = q.eye_n;
            o.flags = (a[(size_t)c].flags & SDR_METER_ROW_AUDIO) | (q.flags & SDR_METER_ROW_RDS);
            sdr_meter_state st{};
            check_sdr(sdr_meter_status(mode, &o, &mo, &st), "sdr_meter_status");
            Sum& s = sum[(size_t)c];
            const double v[5] = {st.offset, st.level_db, st.pilot_nr, st.rds_nr, st.eye_db};
            for (int i = 0; i < 5; i++) s.v[i] += v[i];
            for (int i = 0; i < 4; i++) s.flag[i] += (st.flags >> i) & 1;
        }
        other.pop_front();
        blocks++;
        if (f && std::fwrite(out.data(), sizeof(sdr_meter_row), out.size(), f) != out.size()) die("cannot write the .meter file");
    }
    // PREFIX.status: per channel the run's means and the flags that held on more than half the blocks
    void write_status(const std::string& path) const {
        FILE* t = std::fopen(path.c_str(), "w");
        if (!t) die("cannot write " + path);
        static const char* names[4] = {"STEREO", "RDS", "OFFTUNE", "DEAD_AIR"};
        for (int c = 0; c < nch; c++) {
            const Sum& s = sum[(size_t)c];
            const double n = blocks > 0 ? (double)blocks : 1.0;
            std::fprintf(t, "ch %d: offset %.4f level_db %.2f pilot_nr %.3f rds_nr %.3f eye_db %.2f flags", c, s.v[0] / n,
                         s.v[1] / n, s.v[2] / n, s.v[3] / n, s.v[4] / n);
            bool any = false;
            for (int i = 0; i < 4; i++)
                if (2 * s.flag[i] > blocks) {
                    std::fprintf(t, "%c%s", any ? '|' : ' ', names[i]);
                    any = true;
                }
            std::fprintf(t, "%s\n", any ? "" : " -");
        }
        std::fclose(t);
    }
};

// A finished run's audio side: the stage, its device rows (two, as d_lr) and pinned copies (as h_lr)
struct AudioFin {
    sdr_audio* a = nullptr;
    bool blend = false;                  // the blend targets follow the meter's rows
    int16_t *d_out[2] = {}, *h_out[LAG + 1] = {};
    FILE* f = nullptr;                   // PREFIX.audio
};

struct Shared {
    sdr_multi_opts o{};
    MeterOut* meter = nullptr;           // a metered run (sdr_multi_run_metered)
    AudioFin* fin = nullptr;             // a finished run (sdr_multi_run_finished)
    int rows = 0;                        // input rows per block: nch, a tuned run's nsrc, a wide run's nwide
    bool tuned = false;
    sdr_split* split = nullptr;          // a wide run (sdr_multi_run_wide): the input rows are wide int8 streams
    size_t in_row = 0;                   // bytes of an input row: 2*block_iq, or a wide run's 2*W*block_iq
    int split_rows = 0;                  // a wide run's capture rows per block, nwide * (2 W - 1)
    AudioRes ar;
    RdsRes rr;
    hipStream_t s_d2h = nullptr;         // the L/R copies when not on s_post (SDR_MULTI_D2H=copy)
    sdr_info info{};
    ThreadSafeQueue<FmBatch*> q;
    sdr_ctx* ctx[3] = {};                // RF, audio, RDS (each thread owns its context)
    hipStream_t s_fe = nullptr, s_post = nullptr, s_pll[2] = {}, s_copy = nullptr;
    hipStream_t s_post_c[2] = {};        // consumer i's post stream: s_post, or its own (SDR_MULTI_POSTS=2)
    // persistent mode: a stream over every CU for the first block's front-end side and the last
    // block's post side (the PLL CUs idle then, as bench.py's fill and drain stream), and the events
    // that order the switches (RF, audio, RDS)
    hipStream_t s_all = nullptr;
    hipEvent_t ev_first[3] = {}, ev_last[3] = {};
    // the threads start before the clock: each makes its first runtime calls (per-thread HIP state),
    // reports ready and waits for the go
    std::mutex start_mu;
    std::condition_variable start_cv;
    int ready = 0;
    bool go = false;
    // the pipeline fill: block 1's front end is enqueued only after both consumers have ordered their
    // block 1 pre parts behind block 0's (consumer_pll), so that it runs after block 0's pre parts
    // instead of beside them -- those start the PLLs (SDR_MULTI_FILL=0: no such wait, round 6's first
    // engine; profiles/r06/queue_fill/)
    bool fill_gate = true;
    int first_pre = 0;
    void arrive_and_wait() {
        (void)hipStreamQuery(s_fe);
        std::unique_lock<std::mutex> lk(start_mu);
        ready++;
        start_cv.notify_all();
        start_cv.wait(lk, [this] { return go; });
    }
    bool persistent = false;
    long long nblocks_known = -1;        // -1: a byte stream of unknown length
    long long blocks = 0;
    double read_s = 0.0, h2d_ms = 0.0, d2h_ms = 0.0;   // input reads; GPU time of the H2D / L+R D2H copies
    std::chrono::steady_clock::time_point t_block1{};  // block 1's front end enqueued
};

// block b's front-end-side stream (the all-CU stream for the first block) and consumer i's post stream
// (the all-CU stream for the last block)
hipStream_t fe_stream(const Shared* sh, long long b) { return (sh->s_all && b == 0) ? sh->s_all : sh->s_fe; }
hipStream_t post_stream(const Shared* sh, int i, long long b) {
    return (sh->s_all && b == sh->nblocks_known - 1) ? sh->s_all : sh->s_post_c[i];
}
// work enqueued on `to` from now on follows the work enqueued on `from` so far
void follow(hipStream_t to, hipStream_t from, hipEvent_t ev) {
    check_hip(hipEventRecord(ev, from), "hipEventRecord");
    check_hip(hipStreamWaitEvent(to, ev, 0), "hipStreamWaitEvent");
}

// the host waits for a block's outputs by polling the event (yielding between polls) rather than
// hipEventSynchronize, so a waiting consumer thread never sits inside the runtime while the other
// threads enqueue the next blocks (SDR_MULTI_SYNC=event: hipEventSynchronize, for A/B)
bool g_poll_events = true;
void wait_event(hipEvent_t e) {
    if (!g_poll_events) {
        check_hip(hipEventSynchronize(e), "hipEventSynchronize");
        return;
    }
    for (;;) {
        const hipError_t r = hipEventQuery(e);
        if (r == hipSuccess) return;
        if (r != hipErrorNotReady) check_hip(r, "hipEventQuery");
        std::this_thread::yield();
    }
}

hipEvent_t timing_event() {
    hipEvent_t e = nullptr;
    check_hip(hipEventCreate(&e), "hipEventCreate");
    return e;
}
float elapsed_ms(hipEvent_t a, hipEvent_t b) {
    wait_event(b);
    float ms = 0.0f;
    check_hip(hipEventElapsedTime(&ms, a, b), "hipEventElapsedTime");
    return ms;
}

// ------------------------------------------------------------------ RF front end (producer)
void rf_thread(Shared* sh) {
    const sdr_multi_opts& o = sh->o;
    check_hip(hipSetDevice(o.device), "hipSetDevice");
    sh->arrive_and_wait();
    sdr_ctx* ctx = sh->ctx[0];
    const sdr_info& in = sh->info;
    const size_t row = 2 * (size_t)in.block_iq, bytes = sh->in_row * (size_t)sh->rows;
    hipStream_t s = sh->s_fe;
    const bool dev_in = o.in_path == nullptr;
    uint8_t* d_iq[2] = {};
    hipEvent_t h2d[2] = {}, fe_done[2] = {};
    // copy timing: a ring of event pairs, read without blocking the producer (a pair is waited for
    // only when the ring wraps onto a copy that has not finished)
    constexpr int TR = 8;
    hipEvent_t c0[TR] = {}, c1[TR] = {};
    long long timed = 0;                                    // blocks whose copy time is in h2d_ms
    auto harvest = [&](long long upto, bool wait) {
        for (; timed < upto; timed++) {
            const int t = (int)(timed % TR);
            if (!wait && hipEventQuery(c1[t]) == hipErrorNotReady) break;
            sh->h2d_ms += elapsed_ms(c0[t], c1[t]);
        }
    };
    // a wide run: two buffers of capture rows. Block b's splitter writes buffer b & 1 on the block's
    // front-end stream, in front of the front end that reads it; block b + 2 may be on another stream
    // than block b (the first block's all-CU stream), so its splitter waits for rows_done of block b.
    uint8_t* d_rows[2] = {};
    hipEvent_t rows_done[2] = {};
    if (sh->split)
        for (int k = 0; k < 2; k++) {
            check_hip(hipMalloc(reinterpret_cast<void**>(&d_rows[k]), row * (size_t)sh->split_rows), "hipMalloc");
            rows_done[k] = new_event();
        }
    Reader* rd = nullptr;
    if (!dev_in) {
        for (int k = 0; k < 2; k++) {
            check_hip(hipMalloc(reinterpret_cast<void**>(&d_iq[k]), bytes), "hipMalloc");
            h2d[k] = new_event();
            fe_done[k] = new_event();
        }
        for (int i = 0; i < TR; i++) { c0[i] = timing_event(); c1[i] = timing_event(); }
        rd = new Reader(o.in_path, bytes);
    }
    for (long long b = 0;; b++) {
        const uint8_t* src = nullptr;
        size_t stride = sh->in_row;
        if (dev_in) {
            if (b >= o.nblocks) break;
            src = o.d_iq + (size_t)b * o.block_stride;
            stride = o.row_stride;
        } else {
            const int slot = rd->next();
            if (slot < 0) break;
            const int k = (int)(b & 1);
            if (b >= 2) check_hip(hipStreamWaitEvent(sh->s_copy, fe_done[k], 0), "hipStreamWaitEvent");
            harvest(b - TR + 1, true);                      // the ring slot this block reuses
            harvest(b, false);
            const int t = (int)(b % TR);
            check_hip(hipEventRecord(c0[t], sh->s_copy), "hipEventRecord");
            check_hip(hipMemcpyAsync(d_iq[k], rd->slot[slot], bytes, hipMemcpyHostToDevice, sh->s_copy), "hipMemcpyAsync");
            check_hip(hipEventRecord(c1[t], sh->s_copy), "hipEventRecord");
            check_hip(hipEventRecord(h2d[k], sh->s_copy), "hipEventRecord");
            rd->release(slot, sh->s_copy);
            check_hip(hipStreamWaitEvent(s, h2d[k], 0), "hipStreamWaitEvent");
            src = d_iq[k];
        }
        if (b == 1 && sh->s_all && sh->fill_gate) {   // after both consumers' block 0 pre parts (Shared)
            std::unique_lock<std::mutex> lk(sh->start_mu);
            sh->start_cv.wait(lk, [sh] { return sh->first_pre == 2; });
        }
        if (b == 1) sh->t_block1 = std::chrono::steady_clock::now();
        const hipStream_t sf = fe_stream(sh, b);
        if (!dev_in && sf != s) check_hip(hipStreamWaitEvent(sf, h2d[(int)(b & 1)], 0), "hipStreamWaitEvent");
        if (sh->split) {
            const int k = (int)(b & 1);
            if (b >= 2) check_hip(hipStreamWaitEvent(sf, rows_done[k], 0), "hipStreamWaitEvent");
            check_sdr(sdr_split_block(sh->split, reinterpret_cast<const int8_t*>(src), stride, d_rows[k], row, sf),
                      "sdr_split_block");
            check_sdr(sdr_frontend_tuned(ctx, d_rows[k], row, sf), "sdr_frontend_tuned");
            check_hip(hipEventRecord(rows_done[k], sf), "hipEventRecord");
        } else if (sh->tuned) check_sdr(sdr_frontend_tuned(ctx, src, stride, sf), "sdr_frontend_tuned");
        else check_sdr(sdr_frontend(ctx, src, stride, sf), "sdr_frontend");
        if (!dev_in) check_hip(hipEventRecord(fe_done[(int)(b & 1)], sf), "hipEventRecord");
        FmBatch* fb = sh->q.acquire();
        for (auto& e : fb->released) check_hip(hipStreamWaitEvent(sf, e, 0), "hipStreamWaitEvent");
        check_sdr(sdr_get_fm_demod(ctx, fb->d_fm, fb->stride, sf), "sdr_get_fm_demod");
        check_hip(hipEventRecord(fb->ready, sf), "hipEventRecord");
        if (sf != s) follow(s, sf, sh->ev_first[0]);       // block 1's front end after block 0's
        fb->block = b;
        sh->q.push(fb);                                     // rffrontend.cpp:74
        sh->blocks = b + 1;
    }
    sh->q.push(nullptr);                                    // end of stream
    check_hip(hipStreamSynchronize(s), "hipStreamSynchronize");
    for (int k = 0; k < 2 && sh->split; k++) {
        (void)hipFree(d_rows[k]);
        (void)hipEventDestroy(rows_done[k]);
    }
    if (!dev_in) {
        harvest(sh->blocks, true);
        sh->read_s = rd->read_s;
        delete rd;
        for (auto& p : d_iq) (void)hipFree(p);
        for (int i = 0; i < TR; i++) { (void)hipEventDestroy(c0[i]); (void)hipEventDestroy(c1[i]); }
    }
}

// consumer prologue: the batch into this thread's context (wait_and_pop + prepare, async)
bool consume(Shared* sh, sdr_ctx* ctx, int indicator) {
    FmBatch* fb = nullptr;
    sh->q.wait_and_pop(fb, indicator);
    if (!fb) return false;
    hipStream_t s = fe_stream(sh, fb->block);
    check_hip(hipStreamWaitEvent(s, fb->ready, 0), "hipStreamWaitEvent");
    check_sdr(sdr_push_fm_demod(ctx, fb->d_fm, fb->stride, s), "sdr_push_fm_demod");
    check_hip(hipEventRecord(fb->released[indicator], s), "hipEventRecord");
    sh->q.prepare(indicator);
    return true;
}

// the consumer's PLL of the block whose pre part is on s_fe: signal + wait on s_post (persistent),
// or one dispatch on its own stream between two events
void consumer_pll(Shared* sh, sdr_ctx* ctx, int indicator, hipEvent_t pre, hipEvent_t pll, long long b) {
    if (sh->persistent) {
        const hipStream_t sf = fe_stream(sh, b), sp = post_stream(sh, indicator, b);
        check_sdr(sdr_plls_signal(ctx, sf), "sdr_plls_signal");
        if (sf != sh->s_fe) {
            follow(sh->s_fe, sf, sh->ev_first[1 + indicator]);   // block 1's pre after block 0's
            std::lock_guard<std::mutex> lk(sh->start_mu);
            sh->first_pre++;
            sh->start_cv.notify_all();
        }
        if (sp != sh->s_post_c[indicator]) follow(sp, sh->s_post_c[indicator], sh->ev_last[1 + indicator]);
        check_sdr(sdr_plls_wait(ctx, sp), "sdr_plls_wait");
        return;
    }
    check_hip(hipEventRecord(pre, sh->s_fe), "hipEventRecord");
    check_hip(hipStreamWaitEvent(sh->s_pll[indicator], pre, 0), "hipStreamWaitEvent");
    if (indicator == 0) check_sdr(sdr_stereo_pll(ctx, sh->s_pll[0]), "sdr_stereo_pll");
    else check_sdr(sdr_rds_pll(ctx, sh->s_pll[1]), "sdr_rds_pll");
    check_hip(hipEventRecord(pll, sh->s_pll[indicator]), "hipEventRecord");
    check_hip(hipStreamWaitEvent(sh->s_post_c[indicator], pll, 0), "hipStreamWaitEvent");
}

// ------------------------------------------------------------------ audio (consumer 0)
void audio_thread(Shared* sh) {
    const sdr_multi_opts& o = sh->o;
    check_hip(hipSetDevice(o.device), "hipSetDevice");
    sh->arrive_and_wait();
    sdr_ctx* ctx = sh->ctx[1];
    const size_t n = 2 * (size_t)sh->info.n_audio, bytes = n * o.nch * sizeof(int16_t);
    AudioRes& r = sh->ar;
    FILE* f = nullptr;
    if (o.out_prefix) {
        f = std::fopen((std::string(o.out_prefix) + ".pcm").c_str(), "wb");
        if (!f) die(std::string("cannot write ") + o.out_prefix + ".pcm");
    }
    long long b = 0;
    auto write_block = [&](long long blk) {   // stereo.cpp:111, for every channel
        const int h = (int)(blk % NH);
        wait_event(r.out_ready[h]);
        sh->d2h_ms += elapsed_ms(r.d0[h], r.d1[h]);
        if (sh->meter) sh->meter->part(blk, 0, sh->meter->h_rows[0][h]);
        if (f) std::fwrite(r.h_lr[h], 1, bytes, f);
        if (sh->fin && sh->fin->f && std::fwrite(sh->fin->h_out[h], 1, bytes, sh->fin->f) != bytes)
            die("cannot write the .audio file");
        if (o.cap_lr && blk < o.cap_blocks)
            for (int i = 0; i < o.ncap; i++)
                std::memcpy(o.cap_lr + ((size_t)blk * o.ncap + i) * n, r.h_lr[h] + (size_t)o.cap_ch[i] * n,
                            n * sizeof(int16_t));
    };
    while (consume(sh, ctx, 0)) {
        const int k = (int)(b & 1), h = (int)(b % NH);
        check_sdr(sdr_stereo_pre(ctx, fe_stream(sh, b)), "sdr_stereo_pre");
        consumer_pll(sh, ctx, 0, r.pre, r.pll, b);
        const hipStream_t s = post_stream(sh, 0, b), sc = sh->s_d2h ? sh->s_d2h : s;
        // d_lr[k] is free once block b-2's copy out of it is done (same stream, or the copy stream's event)
        if (sc != s && b >= 2) check_hip(hipStreamWaitEvent(s, r.out_ready[(b - 2) % NH], 0), "hipStreamWaitEvent");
        check_sdr(sdr_stereo_post(ctx, r.d_lr[k], n, s), "sdr_stereo_post");
        if (MeterOut* mt = sh->meter) {
            const sdr_meter_row* d_rows = nullptr;
            check_sdr(sdr_meter_audio(mt->m, ctx, r.d_lr[k], n, s), "sdr_meter_audio");
            check_sdr(sdr_meter_rows(mt->m, &d_rows), "sdr_meter_rows");
            check_hip(hipMemcpyAsync(mt->h_rows[0][h], d_rows, (size_t)o.nch * sizeof(sdr_meter_row), hipMemcpyDeviceToHost, s),
                      "hipMemcpyAsync");
        }
        AudioFin* af = sh->fin;
        if (af) {   // d_out[k] is free as d_lr[k] is: its copy of block b-2 precedes out_ready
            if (af->blend) check_sdr(sdr_audio_blend_from_meter(af->a, sh->meter->m, s), "sdr_audio_blend_from_meter");
            check_sdr(sdr_audio_finish(af->a, r.d_lr[k], n, af->d_out[k], n, s), "sdr_audio_finish");
        }
        if (sc != s) {
            check_hip(hipEventRecord(r.post, s), "hipEventRecord");
            check_hip(hipStreamWaitEvent(sc, r.post, 0), "hipStreamWaitEvent");
        }
        check_hip(hipEventRecord(r.d0[h], sc), "hipEventRecord");
        check_hip(hipMemcpyAsync(r.h_lr[h], r.d_lr[k], bytes, hipMemcpyDeviceToHost, sc), "hipMemcpyAsync");
        check_hip(hipEventRecord(r.d1[h], sc), "hipEventRecord");
        if (af) check_hip(hipMemcpyAsync(af->h_out[h], af->d_out[k], bytes, hipMemcpyDeviceToHost, sc), "hipMemcpyAsync");
        check_hip(hipEventRecord(r.out_ready[h], sc), "hipEventRecord");
        if (b >= LAG) write_block(b - LAG);                 // overlaps the GPU work of blocks b-1, b
        b++;
    }
    for (long long blk = std::max(0LL, b - LAG); blk < b; blk++) write_block(blk);
    if (f) std::fclose(f);
    for (hipStream_t x : {sh->s_post_c[0], sh->s_d2h, sh->s_all})
        if (x) check_hip(hipStreamSynchronize(x), "hipStreamSynchronize");
}

// ------------------------------------------------------------------ RDS (consumer 1)
struct FrameState {   // rds.cpp:67-92, per channel
    uint64_t reg = 0, chars = 0, output = 0;
    bool first_time = true;
    int decoder_cont = 0;
    unsigned int idx = 0;
    std::deque<std::string> window;
    std::vector<int> stream, stream_state;
    std::string text;
};

void rds_thread(Shared* sh) {
    const sdr_multi_opts& o = sh->o;
    check_hip(hipSetDevice(o.device), "hipSetDevice");
    sh->arrive_and_wait();
    sdr_ctx* ctx = sh->ctx[2];
    RdsRes& r = sh->rr;
    hipEvent_t pre = r.pre, pll = r.pll, *out_ready = r.out_ready;   // [NH]
    int32_t *d_nbits = r.d_nbits, **h_nbits = r.h_nbits;
    uint8_t *d_bits = r.d_bits, **h_bits = r.h_bits;
    std::vector<FrameState> fs((size_t)o.nch);
    auto frame_layer = [&](long long blk) {   // rds.cpp:181-189 per channel; parse() prints to cerr
        const int k = (int)(blk % NH);
        wait_event(out_ready[k]);
        if (sh->meter) sh->meter->part(blk, 1, sh->meter->h_rows[1][k]);
        if (o.cap_nbits && blk < o.cap_blocks)
            for (int i = 0; i < o.ncap; i++) {
                o.cap_nbits[(size_t)blk * o.ncap + i] = h_nbits[k][o.cap_ch[i]];
                std::memcpy(o.cap_bits + ((size_t)blk * o.ncap + i) * SDR_MAX_BITS,
                            h_bits[k] + (size_t)o.cap_ch[i] * SDR_MAX_BITS, SDR_MAX_BITS);
            }
        if (!o.out_prefix) return;
        std::streambuf* saved = std::cerr.rdbuf();
        for (int c = 0; c < o.nch; c++) {
            const int nb = h_nbits[k][c];
            if (nb < 0) continue;                       // block_count <= 5 (rds.cpp:135)
            FrameState& st = fs[(size_t)c];
            const uint8_t* bits = h_bits[k] + (size_t)c * SDR_MAX_BITS;
            st.decoder_cont++;
            st.stream.insert(st.stream.end(), bits, bits + nb);
            if (st.decoder_cont == 15) {
                std::ostringstream text;
                std::cerr.rdbuf(text.rdbuf());
                start_frame_sync(st.idx, st.stream, st.stream_state, st.reg, st.chars, st.output, st.first_time,
                                 st.window);
                std::cerr.rdbuf(saved);
                st.text += text.str();
                st.decoder_cont = 0;
                st.idx = 0;
                st.stream.clear();
            }
        }
    };
    long long b = 0;
    while (consume(sh, ctx, 1)) {
        const int k = (int)(b % NH);
        check_sdr(sdr_rds_pre(ctx, fe_stream(sh, b)), "sdr_rds_pre");
        consumer_pll(sh, ctx, 1, pre, pll, b);
        const hipStream_t s = post_stream(sh, 1, b);
        check_sdr(sdr_rds_post(ctx, nullptr, 0, s), "sdr_rds_post");
        if (MeterOut* mt = sh->meter) {
            const sdr_meter_row* d_rows = nullptr;
            check_sdr(sdr_meter_rds(mt->m, ctx, s), "sdr_meter_rds");
            check_sdr(sdr_meter_rows(mt->m, &d_rows), "sdr_meter_rows");
            check_hip(hipMemcpyAsync(mt->h_rows[1][k], d_rows, (size_t)o.nch * sizeof(sdr_meter_row), hipMemcpyDeviceToHost, s),
                      "hipMemcpyAsync");
        }
        check_sdr(sdr_rds_bits(ctx, nullptr, nullptr, nullptr, 0, d_nbits, d_bits, SDR_MAX_BITS, s), "sdr_rds_bits");
        check_hip(hipMemcpyAsync(h_nbits[k], d_nbits, o.nch * sizeof(int32_t), hipMemcpyDeviceToHost, s),
                  "hipMemcpyAsync");
        check_hip(hipMemcpyAsync(h_bits[k], d_bits, (size_t)o.nch * SDR_MAX_BITS, hipMemcpyDeviceToHost, s),
                  "hipMemcpyAsync");
        check_hip(hipEventRecord(out_ready[k], s), "hipEventRecord");
        if (b >= LAG) frame_layer(b - LAG);
        b++;
    }
    for (long long blk = std::max(0LL, b - LAG); blk < b; blk++) frame_layer(blk);
    if (o.out_prefix) {
        FILE* f = std::fopen((std::string(o.out_prefix) + ".rds").c_str(), "w");
        if (!f) die(std::string("cannot write ") + o.out_prefix + ".rds");
        for (int c = 0; c < o.nch; c++) {
            std::istringstream lines(fs[(size_t)c].text);
            for (std::string line; std::getline(lines, line);) std::fprintf(f, "ch %d: %s\n", c, line.c_str());
        }
        std::fclose(f);
    }
    for (hipStream_t x : {sh->s_post_c[1], sh->s_all})
        if (x) check_hip(hipStreamSynchronize(x), "hipStreamSynchronize");
}

// pinned host buffers outlive a run: a process that runs the receiver again (a server taking one input
// after another, bench.py's timed second run) reuses them instead of pinning ~25 MB anew, which took
// ~50 ms in which the GPU sat idle and its clock fell (profiles/r06/queue_fill/). Held until the
// process exits; SDR_MULTI_PIN_CACHE=0: allocated and freed per run.
std::mutex g_pin_mu;
std::vector<std::pair<size_t, void*>> g_pin_free;
bool pin_cache_on() {
    const char* e = std::getenv("SDR_MULTI_PIN_CACHE");
    return !e || std::atoi(e) != 0;
}
template <typename T>
void pinned_get(T** p, size_t bytes) {
    if (pin_cache_on()) {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        for (size_t i = 0; i < g_pin_free.size(); i++)
            if (g_pin_free[i].first == bytes) {
                *p = static_cast<T*>(g_pin_free[i].second);
                g_pin_free.erase(g_pin_free.begin() + (long)i);
                return;
            }
    }
    check_hip(hipHostMalloc(reinterpret_cast<void**>(p), bytes, hipHostMallocDefault), "hipHostMalloc");
}
void pinned_put(void* p, size_t bytes) {
    if (!p) return;
    if (!pin_cache_on()) {
        (void)hipHostFree(p);
        return;
    }
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pin_free.emplace_back(bytes, p);
}

void alloc_consumers(Shared* sh) {
    const sdr_multi_opts& o = sh->o;
    AudioRes& a = sh->ar;
    const size_t lr_bytes = 2 * (size_t)sh->info.n_audio * o.nch * sizeof(int16_t);
    a.pre = new_event();
    a.pll = new_event();
    a.post = new_event();
    for (int k = 0; k < 2; k++) check_hip(hipMalloc(reinterpret_cast<void**>(&a.d_lr[k]), lr_bytes), "hipMalloc");
    for (int h = 0; h < NH; h++) {
        a.out_ready[h] = new_event();
        a.d0[h] = timing_event();
        a.d1[h] = timing_event();
        pinned_get(&a.h_lr[h], lr_bytes);
    }
    RdsRes& r = sh->rr;
    r.pre = new_event();
    r.pll = new_event();
    check_hip(hipMalloc(reinterpret_cast<void**>(&r.d_nbits), o.nch * sizeof(int32_t)), "hipMalloc");
    check_hip(hipMalloc(reinterpret_cast<void**>(&r.d_bits), (size_t)o.nch * SDR_MAX_BITS), "hipMalloc");
    for (int h = 0; h < NH; h++) {
        r.out_ready[h] = new_event();
        pinned_get(&r.h_nbits[h], o.nch * sizeof(int32_t));
        pinned_get(&r.h_bits[h], (size_t)o.nch * SDR_MAX_BITS);
    }
}

void free_consumers(Shared* sh) {
    const sdr_multi_opts& o = sh->o;
    AudioRes& a = sh->ar;
    const size_t lr_bytes = 2 * (size_t)sh->info.n_audio * o.nch * sizeof(int16_t);
    for (hipEvent_t e : {a.pre, a.pll, a.post}) (void)hipEventDestroy(e);
    for (int h = 0; h < NH; h++) {
        for (hipEvent_t e : {a.out_ready[h], a.d0[h], a.d1[h]}) (void)hipEventDestroy(e);
        pinned_put(a.h_lr[h], lr_bytes);
    }
    for (int k = 0; k < 2; k++) (void)hipFree(a.d_lr[k]);
    RdsRes& r = sh->rr;
    for (hipEvent_t e : {r.pre, r.pll}) (void)hipEventDestroy(e);
    (void)hipFree(r.d_nbits);
    (void)hipFree(r.d_bits);
    for (int h = 0; h < NH; h++) {
        (void)hipEventDestroy(r.out_ready[h]);
        pinned_put(r.h_nbits[h], o.nch * sizeof(int32_t));
        pinned_put(r.h_bits[h], (size_t)o.nch * SDR_MAX_BITS);
    }
}

// device-clock period per block of a finished persistent launch, blocks 1 .. last, and the span
// from block 0's start to the last block's end (ms)
void launch_period_ms(sdr_ctx* ctx, hipStream_t s, double* period, double* span, unsigned long long* ends, int nends,
                      bool trace) {
    std::vector<unsigned long long> t0(65536), t1(65536);
    int nb = 0;
    check_sdr(sdr_plls_timeline(ctx, t0.data(), t1.data(), (int)t0.size(), &nb, s), "sdr_plls_timeline");
    if (trace) {   // per block: the PLL's wait for its input (start - previous end) and its duration, us
        std::fprintf(stderr, "sdr_multi: PLL idle/duration us:");
        for (int b = 0; b < nb; b++)
            std::fprintf(stderr, " %.0f/%.0f", b ? ((double)t0[(size_t)b] - (double)t1[(size_t)b - 1]) / 100.0 : 0.0,
                         ((double)t1[(size_t)b] - (double)t0[(size_t)b]) / 100.0);
        std::fprintf(stderr, "\n");
    }
    if (ends)
        for (int b = 0; b < nends && b < nb; b++) ends[b] = t1[(size_t)b];
    if (nb < 2) return;
    *period = std::max(*period, (double)(t1[(size_t)nb - 1] - t1[0]) / (double)(nb - 1) / 1e5);   // 100 MHz ticks
    *span = std::max(*span, (double)(t1[(size_t)nb - 1] - t0[0]) / 1e5);
}

long long regular_file_blocks(const char* path, size_t block_bytes) {
    if (!path || std::strcmp(path, "-") == 0) return -1;
    struct stat sb;
    if (::stat(path, &sb) != 0 || !S_ISREG(sb.st_mode)) return -1;
    return (long long)((size_t)sb.st_size / block_bytes);
}

// the tuning's bounds (sdr_tuner_set's), checked before anything starts
bool tuning_valid(const sdr_multi_opts* o, const sdr_multi_tuning* t) {
    int N = 0;
    if (sdr_tuner_table(o->mode, nullptr, 0, &N) != SDR_OK) return false;
    if (t->nsrc < 1 || t->nsrc > o->nch || !t->src || !t->khz) return false;
    for (int c = 0; c < o->nch; c++)
        if (t->src[c] < 0 || t->src[c] >= t->nsrc || 2 * (long long)t->khz[c] <= -(long long)N ||
            2 * (long long)t->khz[c] > N)
            return false;
    return true;
}

int multi_run(const sdr_multi_opts* opts, const sdr_multi_tuning* tune, const sdr_meter_opts* mo, const sdr_audio_opts* ao,
              bool blend, sdr_multi_stats* stats, const sdr_multi_wide* wide = nullptr) {
    if (!opts || opts->nch <= 0 || (!opts->in_path && (!opts->d_iq || opts->nblocks <= 0)))
        return SDR_E_INVALID;
    if (tune && !tuning_valid(opts, tune)) return SDR_E_INVALID;
    int wide_R = 0, wide_iq = 0;
    if (wide) {   // a wide run is always tuned, on rows the splitter makes
        if (!tune || wide->nwide < 1 || wide->nwide > 4096 || wide->shift > 24 ||
            sdr_split_geometry(opts->mode, wide->W, &wide_R, nullptr, &wide_iq, nullptr, nullptr) != SDR_OK ||
            tune->nsrc > wide->nwide * wide_R)
            return SDR_E_INVALID;
        if (!opts->in_path && ((opts->row_stride & 3) || (reinterpret_cast<uintptr_t>(opts->d_iq) & 3) ||
                               (opts->block_stride & 3) || opts->row_stride < 2 * (size_t)wide_iq))
            return SDR_E_INVALID;
    }
    Shared sh;
    sh.o = *opts;
    sh.tuned = tune != nullptr;
    sh.rows = wide ? wide->nwide : tune ? tune->nsrc : opts->nch;
    const sdr_multi_opts& o = sh.o;
    check_hip(hipSetDevice(o.device), "hipSetDevice");
    // SDR_MULTI_TRACE=1: the set-up and tear-down phases' host times on stderr
    const bool trace = std::getenv("SDR_MULTI_TRACE") && std::atoi(std::getenv("SDR_MULTI_TRACE")) != 0;
    const auto t_call = std::chrono::steady_clock::now();
    auto mark = [&](const char* what) {
        if (trace)
            std::fprintf(stderr, "sdr_multi: %-16s %8.2f ms\n", what,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count());
    };
    sh.ctx[0] = ctx_get(o.device, o.nch, o.mode, 0, o.flags);
    sh.ctx[1] = ctx_get(o.device, o.nch, o.mode, 0, o.flags);
    sh.ctx[2] = ctx_get(o.device, o.nch, o.mode, 1, o.flags);
    mark("contexts");
    // pooled contexts keep their tuning over sdr_ctx_reset: set it on every context of a tuned run,
    // clear it on those of an untuned one
    for (sdr_ctx* c : sh.ctx)
        check_sdr(tune ? sdr_tuner_set(c, tune->nsrc, tune->src, tune->khz, nullptr) : sdr_tuner_set(c, 0, nullptr, nullptr, nullptr),
                  "sdr_tuner_set");
    check_sdr(sdr_ctx_info(sh.ctx[0], &sh.info), "sdr_ctx_info");
    const size_t row = 2 * (size_t)sh.info.block_iq;
    sh.in_row = wide ? 2 * (size_t)wide_iq : row;
    if (!o.in_path && o.row_stride < sh.in_row) {
        for (sdr_ctx* c : sh.ctx) ctx_put(c);
        return SDR_E_INVALID;
    }
    if (wide) {
        sh.split_rows = wide->nwide * wide_R;
        check_sdr(sdr_split_create(&sh.split, o.device, o.mode, wide->W, wide->nwide, wide->shift), "sdr_split_create");
    }
    sh.nblocks_known = o.in_path ? regular_file_blocks(o.in_path, sh.in_row * (size_t)sh.rows) : o.nblocks;
    // streams: the PLLs on [0, pll_cus) (halves), everything else on the rest
    const int half = o.pll_cus / 2;
    if (half > 0) {
        sh.s_fe = masked_stream(o.device, 0, o.pll_cus, 1);
        sh.s_post = masked_stream(o.device, 0, o.pll_cus, 1);
        if (const char* e = std::getenv("SDR_MULTI_POSTS"); e && std::atoi(e) == 2)
            sh.s_post_c[1] = masked_stream(o.device, 0, o.pll_cus, 1);
        sh.s_pll[0] = masked_stream(o.device, 0, half, 0);
        sh.s_pll[1] = masked_stream(o.device, half, half, 0);
        sh.persistent = sh.nblocks_known > 0;
        for (int i = 0; i < 2 && sh.persistent; i++) {   // the library's residency rule (sdr_plls_fits)
            int waves = 0;
            long long groups = 0, resident = 0;
            check_sdr(sdr_plls_fits(sh.ctx[1 + i], i == 0 ? SDR_PLLS_STEREO : SDR_PLLS_RDS, i * half, half, &waves,
                                    &groups, &resident), "sdr_plls_fits");
            sh.persistent = groups <= resident;
        }
        if (sh.persistent) {   // the fill and drain stream (SDR_MULTI_EDGES=0: none)
            const char* ed = std::getenv("SDR_MULTI_EDGES");
            if (!ed || std::atoi(ed) != 0) {
                hipDeviceProp_t prop;
                check_hip(hipGetDeviceProperties(&prop, o.device), "hipGetDeviceProperties");
                sh.s_all = masked_stream(o.device, 0, prop.multiProcessorCount, 0);
                for (int i = 0; i < 3; i++) {
                    sh.ev_first[i] = new_event();
                    sh.ev_last[i] = new_event();
                }
            }
        }
    } else {
        sh.s_fe = plain_stream();
        sh.s_post = plain_stream();
        sh.s_pll[0] = plain_stream();
        sh.s_pll[1] = plain_stream();
    }
    sh.s_post_c[0] = sh.s_post;
    if (!sh.s_post_c[1]) sh.s_post_c[1] = sh.s_post;
    if (o.in_path) sh.s_copy = plain_stream();
    // SDR_MULTI_D2H=copy: the L/R copies on a stream of their own instead of after the post stages
    if (const char* e = std::getenv("SDR_MULTI_D2H"); e && std::strcmp(e, "copy") == 0) sh.s_d2h = plain_stream();
    mark("streams");
    alloc_consumers(&sh);
    MeterOut meter;
    if (mo) {
        meter.mo = *mo;
        meter.nch = o.nch;
        meter.mode = o.mode;
        meter.sum.resize((size_t)o.nch);
        check_sdr(sdr_meter_create(&meter.m, o.device, o.nch, o.mode), "sdr_meter_create");
        for (auto& per : meter.h_rows)
            for (uint8_t*& p : per) pinned_get(&p, (size_t)o.nch * sizeof(sdr_meter_row));
        if (o.out_prefix) {
            meter.f = std::fopen((std::string(o.out_prefix) + ".meter").c_str(), "wb");
            if (!meter.f) die(std::string("cannot write ") + o.out_prefix + ".meter");
        }
        sh.meter = &meter;
    }
    AudioFin fin;
    const size_t fin_bytes = 2 * (size_t)sh.info.n_audio * o.nch * sizeof(int16_t);
    if (ao) {
        fin.blend = blend;
        check_sdr(sdr_audio_create(&fin.a, o.device, o.nch, o.mode, 2, ao), "sdr_audio_create");
        check_sdr(sdr_audio_reset(fin.a, nullptr), "sdr_audio_reset");   // (synchronised with the batches below)
        for (auto& p : fin.d_out) check_hip(hipMalloc(reinterpret_cast<void**>(&p), fin_bytes), "hipMalloc");
        for (auto& p : fin.h_out) pinned_get(&p, fin_bytes);
        if (o.out_prefix) {
            fin.f = std::fopen((std::string(o.out_prefix) + ".audio").c_str(), "wb");
            if (!fin.f) die(std::string("cannot write ") + o.out_prefix + ".audio");
        }
        sh.fin = &fin;
    }
    mark("consumer buffers");
    // two recycled device batches of fm_demod [nch][block_if] (threadsafequeue.h's one slot, plus the
    // one the producer fills meanwhile)
    std::vector<FmBatch> batches(2);
    for (auto& fb : batches) {
        fb.nch = o.nch;
        fb.n = sh.info.block_if;
        fb.stride = (size_t)(fb.n + 63) / 64 * 64;
        check_hip(hipMalloc(reinterpret_cast<void**>(&fb.d_fm), fb.stride * o.nch * sizeof(float)), "hipMalloc");
        fb.ready = new_event();
        for (auto& e : fb.released) {
            e = new_event();
            check_hip(hipEventRecord(e, nullptr), "hipEventRecord");   // trivially complete
        }
        sh.q.add_free(&fb);
    }
    check_hip(hipDeviceSynchronize(), "hipDeviceSynchronize");
    mark("batches");
    // one persistent launch per consumer for every block (before the first sdr_push_fm_demod)
    if (sh.persistent) {
        check_sdr(sdr_plls_launch_sel(sh.ctx[1], (int)sh.nblocks_known, SDR_PLLS_STEREO, sh.s_pll[0]), "sdr_plls_launch_sel");
        check_sdr(sdr_plls_launch_sel(sh.ctx[2], (int)sh.nblocks_known, SDR_PLLS_RDS, sh.s_pll[1]), "sdr_plls_launch_sel");
    }
    if (const char* e = std::getenv("SDR_MULTI_SYNC"); e && std::strcmp(e, "event") == 0) g_poll_events = false;
    if (const char* e = std::getenv("SDR_MULTI_FILL"); e && std::atoi(e) == 0) sh.fill_gate = false;
    std::thread t_rds(rds_thread, &sh);      // project.cpp:134-136
    std::thread t_audio(audio_thread, &sh);
    std::thread t_rf(rf_thread, &sh);
    std::chrono::steady_clock::time_point t0;
    {
        std::unique_lock<std::mutex> lk(sh.start_mu);
        sh.start_cv.wait(lk, [&sh] { return sh.ready == 3; });
        t0 = std::chrono::steady_clock::now();
        mark("threads ready");
        sh.go = true;
        sh.start_cv.notify_all();
    }
    t_rf.join();
    t_audio.join();
    t_rds.join();
    const auto t_end = std::chrono::steady_clock::now();
    mark("run end");
    sdr_multi_stats st{};
    st.blocks = sh.blocks;
    st.seconds = std::chrono::duration<double>(t_end - t0).count();
    st.steady_seconds = sh.blocks >= 2 ? std::chrono::duration<double>(t_end - sh.t_block1).count() : 0.0;
    st.read_s = sh.read_s;
    st.h2d_ms = sh.h2d_ms;
    st.d2h_ms = sh.d2h_ms;
    st.persistent = sh.persistent ? 1 : 0;
    if (sh.persistent) {
        if (sh.blocks != sh.nblocks_known) die("sdr_multi: fewer blocks than the persistent launches cover");
        for (int i = 0; i < 2; i++) {
            double ms[1] = {0.0};
            int nb = 0;
            check_sdr(sdr_plls_report(sh.ctx[1 + i], ms, 0, &nb, sh.s_pll[i]), "sdr_plls_report");   // a timeout fails here
            launch_period_ms(sh.ctx[1 + i], sh.s_pll[i], &st.pll_period_ms, &st.pll_span_ms,
                             o.pll_end ? o.pll_end + (size_t)i * o.stamp_blocks : nullptr, o.stamp_blocks, trace);
        }
    }
    check_hip(hipDeviceSynchronize(), "hipDeviceSynchronize");
    if (sh.split) {
        if (wide->clips) check_sdr(sdr_split_clips(sh.split, wide->clips, nullptr), "sdr_split_clips");
        check_sdr(sdr_split_destroy(sh.split), "sdr_split_destroy");
    }
    for (auto& fb : batches) {
        (void)hipFree(fb.d_fm);
        (void)hipEventDestroy(fb.ready);
        for (auto& e : fb.released) (void)hipEventDestroy(e);
    }
    free_consumers(&sh);
    if (mo) {
        if (meter.f) std::fclose(meter.f);
        if (o.out_prefix) meter.write_status(std::string(o.out_prefix) + ".status");
        for (auto& per : meter.h_rows)
            for (uint8_t* p : per) pinned_put(p, (size_t)o.nch * sizeof(sdr_meter_row));
        check_sdr(sdr_meter_destroy(meter.m), "sdr_meter_destroy");
    }
    if (ao) {
        if (fin.f) std::fclose(fin.f);
        for (auto& p : fin.h_out) pinned_put(p, fin_bytes);
        for (auto& p : fin.d_out) (void)hipFree(p);
        check_sdr(sdr_audio_destroy(fin.a), "sdr_audio_destroy");
    }
    for (sdr_ctx* c : sh.ctx) ctx_put(c);
    if (sh.s_d2h) (void)hipStreamDestroy(sh.s_d2h);
    if (sh.s_post_c[1] != sh.s_post) release_masked(sh.s_post_c[1]);
    if (sh.s_all) release_masked(sh.s_all);
    for (int i = 0; i < 3; i++)
        for (hipEvent_t ev : {sh.ev_first[i], sh.ev_last[i]})
            if (ev) (void)hipEventDestroy(ev);
    for (hipStream_t s : {sh.s_fe, sh.s_post, sh.s_pll[0], sh.s_pll[1]}) {
        if (half > 0) release_masked(s);
        else (void)hipStreamDestroy(s);
    }
    if (sh.s_copy) (void)hipStreamDestroy(sh.s_copy);
    mark("torn down");
    if (stats) *stats = st;
    return SDR_OK;
}

}  // namespace

extern "C" int sdr_multi_run(const sdr_multi_opts* opts, sdr_multi_stats* stats) {
    return multi_run(opts, nullptr, nullptr, nullptr, false, stats);
}

extern "C" int sdr_multi_run_tuned(const sdr_multi_opts* opts, const sdr_multi_tuning* tune, sdr_multi_stats* stats) {
    return multi_run(opts, tune, nullptr, nullptr, false, stats);
}

extern "C" int sdr_multi_run_metered(const sdr_multi_opts* opts, const sdr_multi_tuning* tune, const sdr_meter_opts* mo,
                                     sdr_multi_stats* stats) {
    if (!mo) return SDR_E_INVALID;
    return multi_run(opts, tune, mo, nullptr, false, stats);
}

extern "C" int sdr_multi_run_finished(const sdr_multi_opts* opts, const sdr_multi_tuning* tune, const sdr_meter_opts* mo,
                                      const sdr_audio_opts* ao, int blend, sdr_multi_stats* stats) {
    if (!opts || !ao || (blend && !mo)) return SDR_E_INVALID;
    float a = 0.0f, b = 0.0f;   // what sdr_audio_create would refuse, before anything starts
    if (sdr_audio_coeffs(opts->mode, ao->tau_us, &a, &b) != SDR_OK || !(ao->blend_hi > ao->blend_lo)) return SDR_E_INVALID;
    return multi_run(opts, tune, mo, ao, blend != 0, stats);
}

extern "C" int sdr_multi_run_wide(const sdr_multi_opts* opts, const sdr_multi_wide* wide, const sdr_multi_tuning* tune,
                                  const sdr_meter_opts* mo, const sdr_audio_opts* ao, int blend, sdr_multi_stats* stats) {
    if (!wide) return sdr_multi_run_finished(opts, tune, mo, ao, blend, stats);
    if (!opts || !tune || (blend && (!mo || !ao))) return SDR_E_INVALID;
    if (ao) {   // what sdr_audio_create would refuse, before anything starts (as sdr_multi_run_finished)
        float a = 0.0f, b = 0.0f;
        if (sdr_audio_coeffs(opts->mode, ao->tau_us, &a, &b) != SDR_OK || !(ao->blend_hi > ao->blend_lo)) return SDR_E_INVALID;
    }
    return multi_run(opts, tune, mo, ao, blend != 0, stats, wide);
}
