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
// With SDR_FLAG_IF_ENVELOPE in the options a metered run is RF-metered too: the RF thread's context alone
// gets the flag, and behind each block's front end, on the same stream, the RF thread calls sdr_meter_rf on
// the shared meter and copies the RF rows out (RfOut: PREFIX.rf, and the run-long rows of PREFIX.rfstatus).
// A finished run (include/sdr_multi_audio.h) adds, behind them on the audio thread's post stream,
// sdr_audio_blend_from_meter (with --blend) and sdr_audio_finish from the block's L/R rows into rows of
// its own, copied out behind the L/R copy and written to PREFIX.audio.
// A decoding run (include/sdr_multi_rds.h) adds sdr_rds_groups behind the RDS thread's sdr_rds_bits, on the
// device rows those bits are in; the block's group records are copied out with the bits, the frame layer
// appends them to PREFIX.groups and feeds one sdr_rds_station per channel, and PREFIX.radio is written at
// the end from the stations and the decoder's counters.
// On the tracker's clock (sdr_multi_run_rds_clock) sdr_rds_track_bits runs on the same stream behind the
// block's RRC, on the context's rds_clean row, and sdr_rds_groups reads its bits instead; sdr_rds_bits, its
// copies and the reference frame layer run as before, so PREFIX.rds and the captures do not change.
// Streams (the four-queue budget of DESIGN.md 5): the producer's front end and both consumers' pre
// parts share one stream (s_fe), both consumers' post parts another (s_post), and each consumer's
// PLL has its own CU-masked stream -- with a known block count ONE persistent launch per consumer
// (sdr_plls_launch_sel: the stereo PLL on CUs [0, pll_cus/2), the RDS PLL on [pll_cus/2, pll_cus)),
// signalled from s_fe and waited for on s_post; otherwise one dispatch per block. s_fe and s_post
// run on the CUs the PLLs leave. A consumer's wait on s_post is enqueued after its signal on s_fe
// and its next parity reuse on s_fe after its post on s_post, so no wait on one stream can sit in
// front of the work it waits for on the other.
//
// A run is described once (RunSpec), judged once, before any device call (validate: the stages' own bounds
// through the library's sdr_*_check functions, the engine's rules spelt out), and owns what it
// makes: every event, buffer, stream, context and file is released by the destructor of the object
// that holds it, in the reverse order of declaration.
//
// Environment switches, read once at the start of a run (Switches):
//   SDR_MULTI_READERS=n       pread threads per block of a regular input file (default 8; 1: fread)
//   SDR_MULTI_POSTS=2         the RDS consumer's post part on a stream of its own
//   SDR_MULTI_EDGES=0         no all-CU stream for the first block's front-end side and the last's post side
//   SDR_MULTI_FILL=0          block 1's front end does not wait for the consumers' block 0 pre parts
//   SDR_MULTI_TRACE=1         the set-up and tear-down phases' host times on stderr
//   SDR_MULTI_CTX_CACHE=0     contexts made and destroyed per run instead of pooled
//   SDR_MULTI_STREAM_CACHE=0  CU-masked streams likewise
//   SDR_MULTI_PIN_CACHE=0     pinned output buffers likewise
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>
#include <mutex>
#include <optional>
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
#include "sdr_multi_rds.h"
#include "sdr_multi_tuned.h"
#include "sdr_multi_wide.h"
#include "sdr_multi_wide16.h"
#include "wide_split.h"

using sdrhost::check_hip;
using sdrhost::check_sdr;
using sdrhost::DevBuf;
using sdrhost::die;

namespace {

// ------------------------------------------------------------------ what a run is
struct RunSpec {
    const sdr_multi_opts* o = nullptr;
    const sdr_multi_tuning* tune = nullptr;   // shared captures (sdr_multi_run_tuned)
    const sdr_meter_opts* meter = nullptr;    // the reception meter (sdr_multi_run_metered)
    const sdr_audio_opts* audio = nullptr;    // audio finishing (sdr_multi_run_finished)
    bool blend = false;                       //   its blend targets follow the meter's rows
    const sdr_multi_wide* wide = nullptr;     // wide captures (sdr_multi_run_wide)
    const sdr_multi_rds* rds = nullptr;       // the RDS group decoder (sdr_multi_run_rds)
    int rds_clock = SDR_MULTI_RDS_CLOCK_REF;  //   whose bits it reads (sdr_multi_run_rds_clock)
    const sdr_rds_track_opts* track = nullptr;   // the tracker's options, with SDR_MULTI_RDS_CLOCK_TRACK
    const sdr_rds_soft_opts* soft = nullptr;  // soft decisions on the tracker's clock (sdr_multi_run_rds_soft)
    const sdr_rds_carrier_opts* carrier = nullptr;   // the derotated rows for the tracker (sdr_multi_run_rds_carrier)
    const sdr_wide_fmt* fmt = nullptr;        // int16 wide captures and their gain (sdr_multi_run_wide_fmt)
};

// Everything SDR_E_INVALID stands for, host arithmetic only: nothing exists yet when a run is refused. A stage's
// own bounds are the library's (its _check function, which its create calls too); what is spelt out here is what
// only the engine knows.
bool validate(const RunSpec& r) {
    const sdr_multi_opts* o = r.o;
    if (!o || (r.blend && (!r.meter || !r.audio))) return false;
    if ((o->flags & SDR_FLAG_FAST_FRONTEND) && (o->flags & SDR_FLAG_PHASE_DEMOD)) return false;   // sdr_ctx_create's rule
    if (o->flags & SDR_FLAG_RDS_QUAD) return false;   // the engine sets it itself, on the RDS thread's context (carrier)
    // an RF-metered run: the meter reads the row, and only the exact front ends write it (sdr_ctx_create's rule)
    if ((o->flags & SDR_FLAG_IF_ENVELOPE) && (!r.meter || (o->flags & SDR_FLAG_FAST_FRONTEND))) return false;
    if (r.audio && sdr_audio_opts_check(o->mode, r.audio) != SDR_OK) return false;
    if (o->nch <= 0 || (!o->in_path && (!o->d_iq || o->nblocks <= 0))) return false;
    if (const sdr_multi_rds* d = r.rds) {   // the decoder's record, and a mode with an RDS bit clock
        const sdr_rds_opts ro{d->max_burst, d->loss_blocks};
        if (sdr_rds_opts_check(&ro) != SDR_OK || !sdr_rds_mode_ok(o->mode)) return false;
    }
    if (r.rds_clock != SDR_MULTI_RDS_CLOCK_REF) {   // the tracker feeds the decoder only
        if (r.rds_clock != SDR_MULTI_RDS_CLOCK_TRACK || !r.rds || !r.track) return false;
        if (sdr_rds_track_opts_check(o->mode, r.track) != SDR_OK) return false;
    }
    if (r.soft) {   // only the tracker has reliabilities
        if (r.rds_clock != SDR_MULTI_RDS_CLOCK_TRACK || !r.rds) return false;
        if (sdr_rds_soft_opts_check(r.soft) != SDR_OK) return false;
    }
    if (r.carrier) {   // the tracker reads its rows
        if (r.rds_clock != SDR_MULTI_RDS_CLOCK_TRACK || !r.rds) return false;
        if (sdr_rds_carrier_opts_check(o->mode, r.carrier) != SDR_OK) return false;
    }
    // a tuned run has capture rows: nsrc = 0 is how sdr_tuner_set takes a tuning away
    if (r.tune && (r.tune->nsrc == 0 || sdr_tuner_check(o->mode, o->nch, r.tune->nsrc, r.tune->src, r.tune->khz) != SDR_OK))
        return false;
    int in_iq = 0;   // samples of an input row; left 0 for a mode the scanner does not know: sdr_ctx_create ends that run
    if (const sdr_multi_wide* w = r.wide) {   // a wide run is always tuned, on rows the splitter makes
        int R = 0;
        const bool s16 = sdrhost::wide16(r.fmt);
        if (s16 && sdrhost::wide_fmt_refusal(r.fmt, o->mode, w->W, w->nwide, w->shift)) return false;
        if (!r.tune || (!s16 && sdr_split_check(o->mode, w->W, w->nwide, w->shift) != SDR_OK) ||
            sdr_split_geometry(o->mode, w->W, &R, nullptr, &in_iq, nullptr, nullptr) != SDR_OK || r.tune->nsrc > w->nwide * R)
            return false;
        if (s16) in_iq *= 2;   // (an int16 row is twice the bytes)
        if (!o->in_path && ((o->row_stride & 3) || (reinterpret_cast<uintptr_t>(o->d_iq) & 3) || (o->block_stride & 3))) return false;
    } else {
        if (sdrhost::wide16(r.fmt)) return false;   // int16 rows are wide rows
        (void)sdr_scan_geometry(o->mode, nullptr, nullptr, &in_iq);   // block_iq, the contexts' (sdr_ctx_info)
    }
    return o->in_path || o->row_stride >= 2 * (size_t)in_iq;
}

struct Switches {   // the file's header comment says what each does
    static int num(const char* name, int unset) {
        const char* e = std::getenv(name);
        return e ? std::atoi(e) : unset;
    }
    int readers = std::max(1, num("SDR_MULTI_READERS", 8));
    bool posts2 = num("SDR_MULTI_POSTS", 1) == 2, edges = num("SDR_MULTI_EDGES", 1) != 0;
    bool fill = num("SDR_MULTI_FILL", 1) != 0, trace = num("SDR_MULTI_TRACE", 0) != 0;
    bool ctx_cache = num("SDR_MULTI_CTX_CACHE", 1) != 0, stream_cache = num("SDR_MULTI_STREAM_CACHE", 1) != 0;
    bool pin_cache = num("SDR_MULTI_PIN_CACHE", 1) != 0;
};

// ------------------------------------------------------------------ owners: released where they go out of scope
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy&) = delete;
    void operator=(const NoCopy&) = delete;
};

struct Event : NoCopy {
    hipEvent_t e = nullptr;
    void make(unsigned flags = hipEventDisableTiming) { check_hip(hipEventCreateWithFlags(&e, flags), "hipEventCreate"); }
    void make_timing() { make(hipEventDefault); }
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    operator hipEvent_t() const { return e; }
};

struct File : NoCopy {   // an output file of the run
    FILE* f = nullptr;
    void open(const std::string& path, const char* mode) {
        f = std::fopen(path.c_str(), mode);
        if (!f) die("cannot write " + path);
    }
    ~File() {
        if (f) std::fclose(f);
    }
    operator FILE*() const { return f; }
};

// Idle objects kept for the process's later runs, by key. Contexts, CU-masked streams and pinned
// buffers outlive a run: making and destroying them took ~13 ms (contexts: ~3 ms to make and ~10 ms to
// destroy, against ~1 ms for sdr_ctx_reset), ~70 ms (the six masked streams) and ~50 ms (pinning ~25 MB)
// per run, in which the GPU idled and its clock fell before the next run's first blocks
// (profiles/r06/queue_fill/). A handle below takes an idle object of its key or makes one, and at its end
// gives it back -- or, with its cache switched off, destroys it. Pooled objects live until the process exits.
template <typename Key, typename T>
struct Pool {
    std::mutex mu;
    std::vector<std::pair<Key, T>> idle;
    bool take(const Key& key, T* out) {
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = idle.size(); i-- > 0;)   // the last given first: a run releases in the reverse order of
            if (idle[i].first == key) {          // taking, so the next run has each object in the role it had
                *out = idle[i].second;
                idle.erase(idle.begin() + (long)i);
                return true;
            }
        return false;
    }
    void give(const Key& key, T v) {
        std::lock_guard<std::mutex> lk(mu);
        idle.emplace_back(key, v);
    }
};
Pool<std::array<int, 4>, hipStream_t> g_streams;   // device, first CU, CUs, exclude
Pool<std::array<int, 5>, sdr_ctx*> g_ctxs;         // device, nch, mode, rds_on, flags
Pool<size_t, void*> g_pinned;                      // bytes

struct Stream : NoCopy {
    hipStream_t s = nullptr;
    std::array<int, 4> key{};
    bool masked = false, keep = false;
    void plain() { check_hip(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate"); }
    // on CUs [first, first + n) (exclude = 0) or on every other CU (exclude = 1); its own hardware queue
    void on_cus(int device, int first, int n, int exclude, bool cache) {
        key = {device, first, n, exclude};
        masked = true;
        keep = cache;
        if (g_streams.take(key, &s)) return;
        void* h = nullptr;
        check_sdr(sdr_stream_create_cu_range(&h, device, first, n, exclude), "sdr_stream_create_cu_range");
        s = (hipStream_t)h;
    }
    ~Stream() {   // idle by then
        if (s && masked && keep) g_streams.give(key, s);
        else if (s && masked) (void)sdr_stream_destroy(s);
        else if (s) (void)hipStreamDestroy(s);
    }
    operator hipStream_t() const { return s; }
};

struct Ctx : NoCopy {
    sdr_ctx* c = nullptr;
    std::array<int, 5> key{};
    bool keep = false;
    // a pooled context comes back in the reference's initial state (sdr_ctx_reset)
    void take(int device, int nch, int mode, int rds_on, int flags, bool cache) {
        key = {device, nch, mode, rds_on, flags};
        keep = cache;
        if (g_ctxs.take(key, &c)) check_sdr(sdr_ctx_reset(c, nullptr), "sdr_ctx_reset");
        else check_sdr(sdr_ctx_create(&c, device, nch, mode, rds_on, flags), "sdr_ctx_create");
    }
    ~Ctx() {   // after the run's streams have drained
        if (c && keep) g_ctxs.give(key, c);
        else if (c) sdr_ctx_destroy(c);
    }
    operator sdr_ctx*() const { return c; }
};

template <typename T>
struct Pinned : NoCopy {
    T* p = nullptr;
    size_t bytes = 0;
    bool keep = false;
    void take(size_t n, bool cache) {
        bytes = n;
        keep = cache;
        void* v = nullptr;
        if (!g_pinned.take(n, &v)) check_hip(hipHostMalloc(&v, n, hipHostMallocDefault), "hipHostMalloc");
        p = static_cast<T*>(v);
    }
    ~Pinned() {
        if (p && keep) g_pinned.give(bytes, p);
        else if (p) (void)hipHostFree(p);
    }
    operator T*() const { return p; }
};

// ------------------------------------------------------------------ reader: input -> pinned ring
struct Reader {
    static constexpr int SLOTS = 4;   // pinned input slots: the read of block b+2..b+3 rides out host jitter
    FILE* f = nullptr;
    size_t bytes = 0;
    uint8_t* slot[SLOTS] = {};
    Event consumed[SLOTS];              // the H2D copy out of the slot has completed
    bool armed[SLOTS] = {};
    std::mutex m;
    std::condition_variable cv;
    std::deque<int> filled, empty;
    bool eof = false;
    double read_s = 0.0;                // time spent reading (the input side of the I/O)
    int readers = 1;                    // pread threads per block (regular files)
    long long file_size = 0, offset = 0;
    std::thread th;

    Reader(const std::string& path, size_t block_bytes, int file_readers) : bytes(block_bytes) {
        f = path == "-" ? stdin : std::fopen(path.c_str(), "rb");
        if (!f) die("cannot open " + path);
        struct stat sb;   // a regular file is read by several threads at once (pread of a block's parts)
        if (f != stdin && fstat(fileno(f), &sb) == 0 && S_ISREG(sb.st_mode)) {
            file_size = (long long)sb.st_size;
            readers = file_readers;
        }
        for (int i = 0; i < SLOTS; i++) {
            check_hip(hipHostMalloc(reinterpret_cast<void**>(&slot[i]), bytes, hipHostMallocDefault), "hipHostMalloc");
            consumed[i].make();
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
    Event pre, pll, out_ready[NH], d0[NH], d1[NH];
    DevBuf<int16_t> d_lr[2];
    Pinned<int16_t> h_lr[NH];
    AudioRes(size_t lr_bytes, bool cache) {
        pre.make();
        pll.make();
        for (auto& d : d_lr) d.get(lr_bytes / sizeof(int16_t));
        for (int h = 0; h < NH; h++) {
            out_ready[h].make();
            d0[h].make_timing();
            d1[h].make_timing();
            h_lr[h].take(lr_bytes, cache);
        }
    }
};
struct RdsRes {
    Event pre, pll, out_ready[NH];
    DevBuf<int32_t> d_nbits;
    DevBuf<uint8_t> d_bits;
    Pinned<int32_t> h_nbits[NH];
    Pinned<uint8_t> h_bits[NH];
    // a decoding run (sdr_multi_run_rds): the group decoder and the pinned copies of a block's records
    sdr_rds_dec* dec = nullptr;
    Pinned<sdr_rds_group> h_groups[NH];
    Pinned<int32_t> h_ngroups[NH];
    // ... on the tracker's clock (sdr_multi_run_rds_clock): the tracker and the bits it writes for the decoder
    sdr_rds_track* trk = nullptr;
    DevBuf<int32_t> d_tnbits;
    DevBuf<uint8_t> d_tbits;
    // ... with soft decisions (sdr_multi_run_rds_soft): the tracker's reliabilities of those bits
    DevBuf<uint16_t> d_tsoft;
    // ... on the derotated rows (sdr_multi_run_rds_carrier): the derotator and the rows it writes for the tracker
    sdr_rds_carrier* car = nullptr;
    DevBuf<float> d_rot;
    size_t rot_stride = 0;
    RdsRes(const sdr_multi_opts& o, const sdr_multi_rds* rds, const sdr_rds_track_opts* track, const sdr_rds_soft_opts* soft,
           const sdr_rds_carrier_opts* carrier, int n_rds, bool cache) {
        const int nch = o.nch;
        pre.make();
        pll.make();
        d_nbits.get((size_t)nch);
        d_bits.get((size_t)nch * SDR_MAX_BITS);
        for (int h = 0; h < NH; h++) {
            out_ready[h].make();
            h_nbits[h].take(nch * sizeof(int32_t), cache);
            h_bits[h].take((size_t)nch * SDR_MAX_BITS, cache);
        }
        if (!rds) return;
        const sdr_rds_opts ro{rds->max_burst, rds->loss_blocks};
        if (soft) check_sdr(sdr_rds_dec_create_soft(&dec, o.device, nch, soft), "sdr_rds_dec_create_soft");
        else check_sdr(sdr_rds_dec_create(&dec, o.device, nch, &ro), "sdr_rds_dec_create");
        for (int h = 0; h < NH; h++) {
            h_groups[h].take((size_t)nch * SDR_RDS_MAX_GROUPS * sizeof(sdr_rds_group), cache);
            h_ngroups[h].take(nch * sizeof(int32_t), cache);
        }
        if (!track) return;
        check_sdr(sdr_rds_track_create(&trk, o.device, nch, o.mode, track), "sdr_rds_track_create");
        d_tnbits.get((size_t)nch);
        d_tbits.get((size_t)nch * SDR_MAX_BITS);
        if (soft) d_tsoft.get((size_t)nch * SDR_MAX_BITS);
        if (!carrier) return;
        check_sdr(sdr_rds_carrier_create(&car, o.device, nch, o.mode, carrier), "sdr_rds_carrier_create");
        rot_stride = ((size_t)n_rds + 3) & ~(size_t)3;   // every row on a 16-byte boundary
        d_rot.get((size_t)nch * rot_stride);
    }
    ~RdsRes() {
        if (car) (void)sdr_rds_carrier_destroy(car);
        if (trk) (void)sdr_rds_track_destroy(trk);
        if (dec) (void)sdr_rds_dec_destroy(dec);
    }
};

// A metered run's host side. Each consumer copies the meter's rows out after its own call and takes
// from the copy only the fields that call wrote (the other consumer may be writing its own meanwhile);
// the block's row is complete, and written, when both parts are in. The consumers stay within a few
// blocks of each other (the queue's prepare()), so few parts ever wait.
struct MeterOut {
    sdr_meter* m = nullptr;
    sdr_meter_opts mo{};
    int nch = 0, mode = 0;
    bool phase = false;                  // SDR_FLAG_PHASE_DEMOD: the rows' fm fields are radians (sdr_meter_deviation)
    Pinned<uint8_t> h_rows[2][NH];       // per consumer and rotation slot: nch rows
    File f;                              // PREFIX.meter
    std::mutex mu;
    std::deque<std::pair<long long, std::vector<sdr_meter_row>>> pending[2];
    long long blocks = 0;
    struct Sum {
        double v[5] = {};                // offset, level_db, pilot_nr, rds_nr, eye_db
        long long flag[4] = {};          // blocks with STEREO, RDS, OFFTUNE, DEAD_AIR
        double peak_khz = 0.0, offset_khz = 0.0;   // a phase run: the maximum and the sum over the blocks
    };
    std::vector<Sum> sum;
    MeterOut(const sdr_multi_opts& o, const sdr_meter_opts& opts, bool cache) : mo(opts), nch(o.nch), mode(o.mode),
          phase((o.flags & SDR_FLAG_PHASE_DEMOD) != 0), sum((size_t)o.nch) {
        check_sdr(sdr_meter_create(&m, o.device, o.nch, o.mode), "sdr_meter_create");
        for (auto& per : h_rows)
            for (auto& p : per) p.take((size_t)nch * sizeof(sdr_meter_row), cache);
        if (o.out_prefix) f.open(std::string(o.out_prefix) + ".meter", "wb");
    }
    ~MeterOut() { (void)sdr_meter_destroy(m); }
    // consumer `which` (0 audio, 1 RDS), behind its meter call on s: the rows into its rotation slot h
    void copy_out(int which, int h, hipStream_t s) {
        const sdr_meter_row* d_rows = nullptr;
        check_sdr(sdr_meter_rows(m, &d_rows), "sdr_meter_rows");
        check_hip(hipMemcpyAsync(h_rows[which][h], d_rows, (size_t)nch * sizeof(sdr_meter_row), hipMemcpyDeviceToHost, s),
                  "hipMemcpyAsync");
    }
    // consumer `which` hands in its copy of block blk's rows, once the copy into slot h has completed
    void part(long long blk, int which, int h) {
        std::vector<sdr_meter_row> mine((size_t)nch);
        std::memcpy(mine.data(), h_rows[which][h], (size_t)nch * sizeof(sdr_meter_row));
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
            if (phase) {
                double pk = 0.0, off = 0.0;
                check_sdr(sdr_meter_deviation(mode, &o, &pk, nullptr, &off), "sdr_meter_deviation");
                s.peak_khz = std::max(s.peak_khz, pk);
                s.offset_khz += off;
            }
        }
        other.pop_front();
        blocks++;
        if (f && std::fwrite(out.data(), sizeof(sdr_meter_row), out.size(), f) != out.size()) die("cannot write the .meter file");
    }
    // PREFIX.status: per channel the run's means and the flags that held on more than half the blocks
    void write_status(const std::string& path) const {
        File t;
        t.open(path, "w");
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
            std::fprintf(t, "%s", any ? "" : " -");
            if (phase) std::fprintf(t, " peak_khz %.2f offset_khz %.3f", s.peak_khz, s.offset_khz / n);
            std::fprintf(t, "\n");
        }
    }
};

// An RF-metered run's host side (SDR_FLAG_IF_ENVELOPE, include/sdr_multi_meter.h). Only the RF thread uses it:
// behind block b's front end it enqueues sdr_meter_rf and the copy of the RF rows into ring slot b % NR, and
// handles a slot's rows (PREFIX.rf, the run-long sums) when the ring comes round to it, or at the end.
void wait_event(hipEvent_t e);           // (below, with the streams' helpers)
struct RfOut {
    static constexpr int NR = 8;
    sdr_meter* m = nullptr;              // the run's meter (MeterOut's)
    int nch = 0, mode = 0;
    Pinned<uint8_t> h_rows[NR];          // nch RF rows per slot
    Event copied[NR];
    File f;                              // PREFIX.rf
    long long handled = 0;               // blocks whose rows are written
    struct Sum {                         // the run-long row (include/sdr_amd.h, sdr_meter_rf_status)
        double s = 0.0, q = 0.0;
        long long n = 0;
        float mn = HUGE_VALF, mx = 0.0f;
        int flags = 0;
    };
    std::vector<Sum> sum;
    RfOut(const sdr_multi_opts& o, sdr_meter* meter, bool cache) : m(meter), nch(o.nch), mode(o.mode), sum((size_t)o.nch) {
        for (int i = 0; i < NR; i++) {
            h_rows[i].take((size_t)nch * sizeof(sdr_meter_rf_row), cache);
            copied[i].make();
        }
        if (o.out_prefix) f.open(std::string(o.out_prefix) + ".rf", "wb");
    }
    void handle(long long upto) {
        for (; handled < upto; handled++) {
            const int h = (int)(handled % NR);
            wait_event(copied[h]);
            const sdr_meter_rf_row* rows = reinterpret_cast<const sdr_meter_rf_row*>(h_rows[h].p);
            for (int c = 0; c < nch; c++) {
                const sdr_meter_rf_row& r = rows[c];
                if (!(r.flags & SDR_METER_ROW_RF)) continue;
                Sum& a = sum[(size_t)c];
                a.s += (double)r.env_sum;
                a.q += (double)r.env_sq;
                a.n += r.n;
                a.mn = std::min(a.mn, r.env_min);
                a.mx = std::max(a.mx, r.env_max);
                a.flags |= r.flags;
            }
            if (f && std::fwrite(rows, sizeof(sdr_meter_rf_row), (size_t)nch, f) != (size_t)nch) die("cannot write the .rf file");
        }
    }
    // block b's front end is enqueued on s
    void block(long long b, sdr_ctx* ctx, hipStream_t s) {
        handle(b - NR + 1);              // the slot this block reuses
        check_sdr(sdr_meter_rf(m, ctx, s), "sdr_meter_rf");
        const sdr_meter_rf_row* d_rows = nullptr;
        check_sdr(sdr_meter_rf_rows(m, &d_rows), "sdr_meter_rf_rows");
        const int h = (int)(b % NR);
        check_hip(hipMemcpyAsync(h_rows[h].p, d_rows, (size_t)nch * sizeof(sdr_meter_rf_row), hipMemcpyDeviceToHost, s),
                  "hipMemcpyAsync");
        check_hip(hipEventRecord(copied[h], s), "hipEventRecord");
    }
    // PREFIX.rfstatus: per channel the run-long row's readings under the default options
    void write_status(const std::string& path) const {
        File t;
        t.open(path, "w");
        sdr_meter_rf_opts ro{};
        sdr_meter_rf_opts_default(&ro);
        for (int c = 0; c < nch; c++) {
            Sum a = sum[(size_t)c];
            while (a.n > INT32_MAX) {    // (the row's n is an int32: halve the three sums, the means stay)
                a.s *= 0.5;
                a.q *= 0.5;
                a.n /= 2;
            }
            sdr_meter_rf_row r{};
            if (a.flags) r = sdr_meter_rf_row{(float)a.s, (float)a.q, a.mn, a.mx, (int32_t)a.n, a.flags, {0, 0}};
            sdr_meter_rf_state st{};
            check_sdr(sdr_meter_rf_status(mode, &r, &ro, &st), "sdr_meter_rf_status");
            std::fprintf(t, "ch %d: level_dbfs %.3f ripple %.3f cnr_db %.3f fade_db %.3f crest_db %.3f flags %s\n", c,
                         st.level_dbfs, st.ripple, st.cnr_db, st.fade_db, st.crest_db,
                         (st.flags & SDR_METER_RF_WEAK) ? "WEAK" : "-");
        }
    }
};

// A finished run's audio side: the stage, its device rows (two, as d_lr) and pinned copies (as h_lr)
struct AudioFin {
    sdr_audio* a = nullptr;
    bool blend = false;                  // the blend targets follow the meter's rows
    DevBuf<int16_t> d_out[2];
    Pinned<int16_t> h_out[NH];
    File f;                              // PREFIX.audio
    AudioFin(const sdr_multi_opts& o, const sdr_audio_opts& ao, bool blend_, size_t lr_bytes, bool cache) : blend(blend_) {
        check_sdr(sdr_audio_create(&a, o.device, o.nch, o.mode, 2, &ao), "sdr_audio_create");
        check_sdr(sdr_audio_reset(a, nullptr), "sdr_audio_reset");   // (synchronised with the batches, before the threads start)
        for (auto& d : d_out) d.get(lr_bytes / sizeof(int16_t));
        for (auto& p : h_out) p.take(lr_bytes, cache);
        if (o.out_prefix) f.open(std::string(o.out_prefix) + ".audio", "wb");
    }
    ~AudioFin() { (void)sdr_audio_destroy(a); }
};

// the code of a call of the wide run's splitter (host/wide_split.h), behind the name of the C call that failed
void check_split(const sdrhost::WideSplit& s, int rc) { check_sdr(rc, s.failed); }

// a recycled device batch of fm_demod [nch][block_if] and its events (include/dropin/fm_batch.h)
struct Batch {
    FmBatch fb;
    DevBuf<float> d_fm;
    Event ready, released[2];
    Batch(int nch, int n) {
        fb.nch = nch;
        fb.n = n;
        fb.stride = (size_t)(n + 63) / 64 * 64;
        fb.d_fm = d_fm.get(fb.stride * nch);
        ready.make();
        fb.ready = ready;
        for (int i = 0; i < 2; i++) {
            released[i].make();
            fb.released[i] = released[i];
            check_hip(hipEventRecord(released[i], nullptr), "hipEventRecord");   // trivially complete
        }
    }
};

struct Trace {   // SDR_MULTI_TRACE=1: a phase's end, in host time since the call
    bool on = false;
    std::chrono::steady_clock::time_point t_call = std::chrono::steady_clock::now();
    void operator()(const char* what) const {
        if (on)
            std::fprintf(stderr, "sdr_multi: %-16s %8.2f ms\n", what,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count());
    }
};

// What the three threads share. Members are released in the reverse of this order: the streams and the
// contexts last.
struct Shared : NoCopy {
    explicit Shared(const Switches& s) : sw(s) {}
    sdr_multi_opts o{};
    const Switches sw;
    int rows = 0;                        // input rows per block: nch, a tuned run's nsrc, a wide run's nwide
    bool tuned = false;
    size_t in_row = 0;                   // bytes of an input row: 2*block_iq, or a wide run's 2*W*block_iq
    sdr_info info{};
    // s_fe, s_post, s_pll: the header comment's streams; s_post2: the RDS consumer's own post stream
    // (SDR_MULTI_POSTS=2); s_copy: the uploads of a byte-stream input
    Stream s_fe, s_post, s_post2, s_pll[2], s_copy;
    hipStream_t s_post_c[2] = {};        // consumer i's post stream: s_post, or s_post2
    // persistent mode: a stream over every CU for the first block's front-end side and the last
    // block's post side (the PLL CUs idle then, as bench.py's fill and drain stream), and the events
    // that order the switches (RF, audio, RDS)
    Stream s_all;
    Event ev_first[3], ev_last[3];
    Ctx ctx[3];                          // RF, audio, RDS (each thread owns its context)
    std::optional<sdrhost::WideSplit> split;   // a wide run: the input rows are wide int8 or int16 streams
    std::optional<AudioRes> ar;
    std::optional<RdsRes> rr;
    std::optional<MeterOut> meter;       // a metered run
    std::optional<RfOut> rf;             // an RF-metered run (the RF thread's)
    std::optional<AudioFin> fin;         // a finished run
    ThreadSafeQueue<FmBatch*> q;
    std::deque<Batch> batches;
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
hipStream_t fe_stream(const Shared* sh, long long b) { return (sh->s_all.s && b == 0) ? sh->s_all.s : sh->s_fe.s; }
hipStream_t post_stream(const Shared* sh, int i, long long b) {
    return (sh->s_all.s && b == sh->nblocks_known - 1) ? sh->s_all.s : sh->s_post_c[i];
}
// work enqueued on `to` from now on follows the work enqueued on `from` so far
void follow(hipStream_t to, hipStream_t from, hipEvent_t ev) {
    check_hip(hipEventRecord(ev, from), "hipEventRecord");
    check_hip(hipStreamWaitEvent(to, ev, 0), "hipStreamWaitEvent");
}

// the host waits for a block's outputs by polling the event (yielding between polls) rather than
// hipEventSynchronize, so a waiting consumer thread never sits inside the runtime while the other
// threads enqueue the next blocks
void wait_event(hipEvent_t e) {
    for (;;) {
        const hipError_t r = hipEventQuery(e);
        if (r == hipSuccess) return;
        if (r != hipErrorNotReady) check_hip(r, "hipEventQuery");
        std::this_thread::yield();
    }
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
    DevBuf<uint8_t> d_iq[2];
    Event h2d[2], fe_done[2];
    // copy timing: a ring of event pairs, read without blocking the producer (a pair is waited for
    // only when the ring wraps onto a copy that has not finished)
    constexpr int TR = 8;
    Event c0[TR], c1[TR];
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
    DevBuf<uint8_t> d_rows[2];
    Event rows_done[2];
    if (sh->split)
        for (int k = 0; k < 2; k++) {
            d_rows[k].get(row * (size_t)sh->split->rows);
            rows_done[k].make();
        }
    std::optional<Reader> rd;
    if (!dev_in) {
        for (int k = 0; k < 2; k++) {
            d_iq[k].get(bytes);
            h2d[k].make();
            fe_done[k].make();
        }
        for (int i = 0; i < TR; i++) {
            c0[i].make_timing();
            c1[i].make_timing();
        }
        rd.emplace(o.in_path, bytes, sh->sw.readers);
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
            check_hip(hipMemcpyAsync(d_iq[k].p, rd->slot[slot], bytes, hipMemcpyHostToDevice, sh->s_copy), "hipMemcpyAsync");
            check_hip(hipEventRecord(c1[t], sh->s_copy), "hipEventRecord");
            check_hip(hipEventRecord(h2d[k], sh->s_copy), "hipEventRecord");
            rd->release(slot, sh->s_copy);
            check_hip(hipStreamWaitEvent(s, h2d[k], 0), "hipStreamWaitEvent");
            src = d_iq[k].p;
        }
        if (b == 1 && sh->s_all.s && sh->sw.fill) {   // after both consumers' block 0 pre parts (Shared)
            std::unique_lock<std::mutex> lk(sh->start_mu);
            sh->start_cv.wait(lk, [sh] { return sh->first_pre == 2; });
        }
        if (b == 1) sh->t_block1 = std::chrono::steady_clock::now();
        const hipStream_t sf = fe_stream(sh, b);
        if (!dev_in && sf != s) check_hip(hipStreamWaitEvent(sf, h2d[(int)(b & 1)], 0), "hipStreamWaitEvent");
        if (sh->split) {
            const int k = (int)(b & 1);
            if (b >= 2) check_hip(hipStreamWaitEvent(sf, rows_done[k], 0), "hipStreamWaitEvent");
            if (b == 0 && sh->split->auto_target >= 0)   // (scratch: the buffer block 1 writes)
                check_split(*sh->split, sh->split->gain_from(src, stride, d_rows[1].p, row, sf));
            check_split(*sh->split, sh->split->block(src, stride, d_rows[k].p, row, sf));
            check_sdr(sdr_frontend_tuned(ctx, d_rows[k].p, row, sf), "sdr_frontend_tuned");
            check_hip(hipEventRecord(rows_done[k], sf), "hipEventRecord");
        } else if (sh->tuned) check_sdr(sdr_frontend_tuned(ctx, src, stride, sf), "sdr_frontend_tuned");
        else check_sdr(sdr_frontend(ctx, src, stride, sf), "sdr_frontend");
        if (sh->rf) sh->rf->block(b, ctx, sf);
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
    check_hip(hipStreamSynchronize(s), "hipStreamSynchronize");   // before this thread's buffers go
    if (sh->rf) sh->rf->handle(sh->blocks);
    if (!dev_in) {
        harvest(sh->blocks, true);
        sh->read_s = rd->read_s;
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

// a consumer's loop: enqueue block b's work, then handle on the host the outputs of block b - LAG (the
// rotation over NH slots); at the end of the stream the last LAG blocks, and the consumer's streams drain
template <typename Enqueue, typename Handle>
void consumer_loop(Shared* sh, sdr_ctx* ctx, int indicator, Enqueue enqueue, Handle handle) {
    long long b = 0;
    for (; consume(sh, ctx, indicator); b++) {
        enqueue(b);
        if (b >= LAG) handle(b - LAG);                      // overlaps the GPU work of blocks b-1, b
    }
    for (long long blk = std::max(0LL, b - LAG); blk < b; blk++) handle(blk);
    for (hipStream_t x : {sh->s_post_c[indicator], sh->s_all.s})
        if (x) check_hip(hipStreamSynchronize(x), "hipStreamSynchronize");
}

// ------------------------------------------------------------------ audio (consumer 0)
void audio_thread(Shared* sh) {
    const sdr_multi_opts& o = sh->o;
    check_hip(hipSetDevice(o.device), "hipSetDevice");
    sh->arrive_and_wait();
    sdr_ctx* ctx = sh->ctx[1];
    const size_t n = 2 * (size_t)sh->info.n_audio, bytes = n * o.nch * sizeof(int16_t);
    AudioRes& r = *sh->ar;
    MeterOut* mt = sh->meter ? &*sh->meter : nullptr;
    AudioFin* af = sh->fin ? &*sh->fin : nullptr;
    File f;
    if (o.out_prefix) f.open(std::string(o.out_prefix) + ".pcm", "wb");
    auto enqueue = [&](long long b) {
        const int k = (int)(b & 1), h = (int)(b % NH);
        check_sdr(sdr_stereo_pre(ctx, fe_stream(sh, b)), "sdr_stereo_pre");
        consumer_pll(sh, ctx, 0, r.pre, r.pll, b);
        const hipStream_t s = post_stream(sh, 0, b);
        // d_lr[k] is free: block b-2's copy out of it precedes on the post stream
        check_sdr(sdr_stereo_post(ctx, r.d_lr[k].p, n, s), "sdr_stereo_post");
        if (mt) {
            check_sdr(sdr_meter_audio(mt->m, ctx, r.d_lr[k].p, n, s), "sdr_meter_audio");
            mt->copy_out(0, h, s);
        }
        if (af) {   // d_out[k] is free as d_lr[k] is: its copy of block b-2 precedes out_ready
            if (af->blend) check_sdr(sdr_audio_blend_from_meter(af->a, mt->m, s), "sdr_audio_blend_from_meter");
            check_sdr(sdr_audio_finish(af->a, r.d_lr[k].p, n, af->d_out[k].p, n, s), "sdr_audio_finish");
        }
        check_hip(hipEventRecord(r.d0[h], s), "hipEventRecord");
        check_hip(hipMemcpyAsync(r.h_lr[h], r.d_lr[k].p, bytes, hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
        check_hip(hipEventRecord(r.d1[h], s), "hipEventRecord");
        if (af) check_hip(hipMemcpyAsync(af->h_out[h], af->d_out[k].p, bytes, hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
        check_hip(hipEventRecord(r.out_ready[h], s), "hipEventRecord");
    };
    auto write_block = [&](long long blk) {   // stereo.cpp:111, for every channel
        const int h = (int)(blk % NH);
        wait_event(r.out_ready[h]);
        sh->d2h_ms += elapsed_ms(r.d0[h], r.d1[h]);
        if (mt) mt->part(blk, 0, h);
        if (f) std::fwrite(r.h_lr[h], 1, bytes, f);
        if (af && af->f && std::fwrite(af->h_out[h], 1, bytes, af->f) != bytes) die("cannot write the .audio file");
        if (o.cap_lr && blk < o.cap_blocks)
            for (int i = 0; i < o.ncap; i++)
                std::memcpy(o.cap_lr + ((size_t)blk * o.ncap + i) * n, r.h_lr[h].p + (size_t)o.cap_ch[i] * n, n * sizeof(int16_t));
    };
    consumer_loop(sh, ctx, 0, enqueue, write_block);
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
    RdsRes& r = *sh->rr;
    MeterOut* mt = sh->meter ? &*sh->meter : nullptr;
    std::vector<FrameState> fs((size_t)o.nch);
    // a decoding run: every channel's station, and PREFIX.groups as the blocks come in
    std::vector<sdr_rds_station> stations(r.dec ? (size_t)o.nch : 0);
    for (auto& st : stations) sdr_rds_station_init(&st);
    File groups;
    if (r.dec && o.out_prefix) groups.open(std::string(o.out_prefix) + ".groups", "w");
    auto enqueue = [&](long long b) {
        const int k = (int)(b % NH);
        check_sdr(sdr_rds_pre(ctx, fe_stream(sh, b)), "sdr_rds_pre");
        consumer_pll(sh, ctx, 1, r.pre, r.pll, b);
        const hipStream_t s = post_stream(sh, 1, b);
        check_sdr(sdr_rds_post(ctx, nullptr, 0, s), "sdr_rds_post");
        if (mt) {
            check_sdr(sdr_meter_rds(mt->m, ctx, s), "sdr_meter_rds");
            mt->copy_out(1, k, s);
        }
        check_sdr(sdr_rds_bits(ctx, nullptr, nullptr, nullptr, 0, r.d_nbits.p, r.d_bits.p, SDR_MAX_BITS, s), "sdr_rds_bits");
        check_hip(hipMemcpyAsync(r.h_nbits[k], r.d_nbits.p, o.nch * sizeof(int32_t), hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
        check_hip(hipMemcpyAsync(r.h_bits[k], r.d_bits.p, (size_t)o.nch * SDR_MAX_BITS, hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
        if (r.trk) {   // the block's rds_clean row, behind its RRC on this stream, into bits of the same layout
            const float* clean = nullptr;
            size_t clean_stride = 0;
            int n_rds = 0;
            check_sdr(sdr_ctx_buffer(ctx, "rds_clean", &clean, &clean_stride, &n_rds), "sdr_ctx_buffer");
            if (r.car) {   // both branches' rows onto one axis first: the tracker reads the rotated rows
                const float* clean_q = nullptr;
                size_t q_stride = 0;
                int n_q = 0;
                check_sdr(sdr_ctx_rds_clean_q(ctx, &clean_q, &q_stride, &n_q), "sdr_ctx_rds_clean_q");
                check_sdr(sdr_rds_carrier_rotate(r.car, clean, clean_stride, clean_q, q_stride, n_rds, r.d_rot.p, r.rot_stride, s),
                          "sdr_rds_carrier_rotate");
                clean = r.d_rot.p;
                clean_stride = r.rot_stride;
            }
            if (r.d_tsoft.p)
                check_sdr(sdr_rds_track_bits_soft(r.trk, clean, clean_stride, n_rds, r.d_tnbits.p, r.d_tbits.p, SDR_MAX_BITS,
                                                  r.d_tsoft.p, SDR_MAX_BITS, s),
                          "sdr_rds_track_bits_soft");
            else
                check_sdr(sdr_rds_track_bits(r.trk, clean, clean_stride, n_rds, r.d_tnbits.p, r.d_tbits.p, SDR_MAX_BITS, s),
                          "sdr_rds_track_bits");
        }
        if (r.dec) {   // on the bits where they are; the last block's stream follows the others' (consumer_pll)
            const int32_t* nbits = r.trk ? r.d_tnbits.p : r.d_nbits.p;
            const uint8_t* bits = r.trk ? r.d_tbits.p : r.d_bits.p;
            if (r.d_tsoft.p)
                check_sdr(sdr_rds_groups_soft(r.dec, nbits, bits, SDR_MAX_BITS, r.d_tsoft.p, SDR_MAX_BITS, s), "sdr_rds_groups_soft");
            else check_sdr(sdr_rds_groups(r.dec, nbits, bits, SDR_MAX_BITS, s), "sdr_rds_groups");
            check_sdr(sdr_rds_groups_copy(r.dec, r.h_groups[k], r.h_ngroups[k], s), "sdr_rds_groups_copy");
        }
        check_hip(hipEventRecord(r.out_ready[k], s), "hipEventRecord");
    };
    auto frame_layer = [&](long long blk) {   // rds.cpp:181-189 per channel; parse() prints to cerr
        const int k = (int)(blk % NH);
        const int32_t* h_nbits = r.h_nbits[k];
        const uint8_t* h_bits = r.h_bits[k];
        wait_event(r.out_ready[k]);
        if (mt) mt->part(blk, 1, k);
        if (o.cap_nbits && blk < o.cap_blocks)
            for (int i = 0; i < o.ncap; i++) {
                o.cap_nbits[(size_t)blk * o.ncap + i] = h_nbits[o.cap_ch[i]];
                std::memcpy(o.cap_bits + ((size_t)blk * o.ncap + i) * SDR_MAX_BITS, h_bits + (size_t)o.cap_ch[i] * SDR_MAX_BITS,
                            SDR_MAX_BITS);
            }
        if (r.dec)
            for (int c = 0; c < o.nch; c++) {
                const int ng = std::min(std::max(r.h_ngroups[k][c], 0), SDR_RDS_MAX_GROUPS);
                for (int j = 0; j < ng; j++) {
                    const sdr_rds_group& g = r.h_groups[k][(size_t)c * SDR_RDS_MAX_GROUPS + j];
                    sdr_rds_station_update(&stations[(size_t)c], &g);
                    if (!groups) continue;
                    std::fprintf(groups, "ch %d bits %u", c, g.bits);
                    for (int w = 0; w < 4; w++) {
                        if (!((g.ok >> w) & 1)) std::fprintf(groups, " ----");
                        else   // a block the soft step placed ends in "~", one the burst table corrected in "*"
                            std::fprintf(groups, " %04X%s", g.w[w],
                                         ((g.flags >> (SDR_RDS_GROUP_SOFT_SHIFT + w)) & 1) ? "~" : ((g.corrected >> w) & 1) ? "*" : "");
                    }
                    std::fprintf(groups, "\n");
                }
            }
        if (!o.out_prefix) return;
        std::streambuf* saved = std::cerr.rdbuf();
        for (int c = 0; c < o.nch; c++) {
            const int nb = h_nbits[c];
            if (nb < 0) continue;                       // block_count <= 5 (rds.cpp:135)
            FrameState& st = fs[(size_t)c];
            const uint8_t* bits = h_bits + (size_t)c * SDR_MAX_BITS;
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
    consumer_loop(sh, ctx, 1, enqueue, frame_layer);
    if (!o.out_prefix) return;
    if (r.dec) {   // PREFIX.radio: what every station said, and how well it was received
        std::vector<sdr_rds_stats> stats((size_t)o.nch);
        check_sdr(sdr_rds_stats_read(r.dec, stats.data(), sh->s_post_c[1]), "sdr_rds_stats_read");
        std::vector<sdr_rds_track_stats> clock(r.trk ? (size_t)o.nch : 0);
        if (r.trk) check_sdr(sdr_rds_track_stats_read(r.trk, clock.data(), sh->s_post_c[1]), "sdr_rds_track_stats_read");
        std::vector<sdr_rds_soft_stats> soft(r.d_tsoft.p ? (size_t)o.nch : 0);
        if (r.d_tsoft.p) check_sdr(sdr_rds_soft_stats_read(r.dec, soft.data(), sh->s_post_c[1]), "sdr_rds_soft_stats_read");
        std::vector<sdr_rds_carrier_stats> carrier(r.car ? (size_t)o.nch : 0);
        if (r.car) check_sdr(sdr_rds_carrier_stats_read(r.car, carrier.data(), sh->s_post_c[1]), "sdr_rds_carrier_stats_read");
        File radio;
        radio.open(std::string(o.out_prefix) + ".radio", "w");
        std::vector<char> buf(4096);
        for (int c = 0; c < o.nch; c++) {
            sdr_rds_station_stats(&stations[(size_t)c], &stats[(size_t)c]);
            sdr_rds_station_format(&stations[(size_t)c], buf.data(), buf.size());
            std::istringstream lines(buf.data());
            for (std::string line; std::getline(lines, line);) std::fprintf(radio, "ch %d: %s\n", c, line.c_str());
            if (!r.trk) continue;
            const sdr_rds_track_stats& k = clock[(size_t)c];
            std::fprintf(radio, "ch %d: clock: locked %u phase %u bits %u moves %u half_moves %u resets %u level %u\n", c, k.locked,
                         k.phase, k.bits, k.moves, k.half_moves, k.resets, k.level);
            if (r.car) {   // the phase in degrees, and hypot(sr, si) / st: 1 for a clean subcarrier, near 0 for noise
                const sdr_rds_carrier_stats& q = carrier[(size_t)c];
                const double coherence = q.st > 0 ? std::hypot((double)q.sr, (double)q.si) / (double)q.st : 0.0;
                std::fprintf(radio, "ch %d: carrier: phase %.2f coherence %.3f windows %u resets %u\n", c,
                             (double)q.phi * (360.0 / 4294967296.0), coherence, q.windows, q.resets);
            }
            if (r.d_tsoft.p)
                std::fprintf(radio, "ch %d: soft: blocks %u flips %u\n", c, soft[(size_t)c].soft_blocks, soft[(size_t)c].soft_flips);
        }
    }
    File f;
    f.open(std::string(o.out_prefix) + ".rds", "w");
    for (int c = 0; c < o.nch; c++) {
        std::istringstream lines(fs[(size_t)c].text);
        for (std::string line; std::getline(lines, line);) std::fprintf(f, "ch %d: %s\n", c, line.c_str());
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

// a validated run, from its set-up to the last output; everything it made is released when it returns
void run(const RunSpec& spec, const Switches& sw, const Trace& mark, sdr_multi_stats* st) {
    Shared sh(sw);
    sh.o = *spec.o;
    sh.tuned = spec.tune != nullptr;
    sh.rows = spec.wide ? spec.wide->nwide : spec.tune ? spec.tune->nsrc : spec.o->nch;
    const sdr_multi_opts& o = sh.o;
    // (the RDS thread's context alone runs the quadrature branch, and only in a run that derotates; the RF thread's
    // alone has a front end, and with it the IF envelope row of an RF-metered run)
    for (int i = 0; i < 3; i++)
        sh.ctx[i].take(o.device, o.nch, o.mode, i == 2,
                       (i == 0 ? o.flags : o.flags & ~SDR_FLAG_IF_ENVELOPE) | (i == 2 && spec.carrier ? SDR_FLAG_RDS_QUAD : 0),
                       sw.ctx_cache);
    mark("contexts");
    // pooled contexts keep their tuning over sdr_ctx_reset: set it on every context of a tuned run,
    // clear it on those of an untuned one
    for (sdr_ctx* c : sh.ctx)
        check_sdr(spec.tune ? sdr_tuner_set(c, spec.tune->nsrc, spec.tune->src, spec.tune->khz, nullptr)
                            : sdr_tuner_set(c, 0, nullptr, nullptr, nullptr), "sdr_tuner_set");
    check_sdr(sdr_ctx_info(sh.ctx[0], &sh.info), "sdr_ctx_info");
    if (const sdr_multi_wide* w = spec.wide) {
        sh.split.emplace();
        check_split(*sh.split, sh.split->open(o.device, o.mode, w->W, w->nwide, w->shift, spec.fmt, nullptr));
    }
    sh.in_row = spec.wide ? sh.split->in_row : 2 * (size_t)sh.info.block_iq;
    sh.nblocks_known = o.in_path ? regular_file_blocks(o.in_path, sh.in_row * (size_t)sh.rows) : o.nblocks;
    // streams: the PLLs on [0, pll_cus) (halves), everything else on the rest
    const int half = o.pll_cus / 2;
    if (half > 0) {
        sh.s_fe.on_cus(o.device, 0, o.pll_cus, 1, sw.stream_cache);
        sh.s_post.on_cus(o.device, 0, o.pll_cus, 1, sw.stream_cache);
        if (sw.posts2) sh.s_post2.on_cus(o.device, 0, o.pll_cus, 1, sw.stream_cache);
        sh.s_pll[0].on_cus(o.device, 0, half, 0, sw.stream_cache);
        sh.s_pll[1].on_cus(o.device, half, half, 0, sw.stream_cache);
        sh.persistent = sh.nblocks_known > 0;
        for (int i = 0; i < 2 && sh.persistent; i++) {   // the library's residency rule (sdr_plls_fits)
            int waves = 0;
            long long groups = 0, resident = 0;
            check_sdr(sdr_plls_fits(sh.ctx[1 + i], i == 0 ? SDR_PLLS_STEREO : SDR_PLLS_RDS, i * half, half, &waves,
                                    &groups, &resident), "sdr_plls_fits");
            sh.persistent = groups <= resident;
        }
        if (sh.persistent && sw.edges) {   // the fill and drain stream
            hipDeviceProp_t prop;
            check_hip(hipGetDeviceProperties(&prop, o.device), "hipGetDeviceProperties");
            sh.s_all.on_cus(o.device, 0, prop.multiProcessorCount, 0, sw.stream_cache);
            for (int i = 0; i < 3; i++) {
                sh.ev_first[i].make();
                sh.ev_last[i].make();
            }
        }
    } else {
        for (Stream* s : {&sh.s_fe, &sh.s_post, &sh.s_pll[0], &sh.s_pll[1]}) s->plain();
    }
    sh.s_post_c[0] = sh.s_post;
    sh.s_post_c[1] = sh.s_post2.s ? sh.s_post2.s : sh.s_post.s;
    if (o.in_path) sh.s_copy.plain();
    mark("streams");
    const size_t lr_bytes = 2 * (size_t)sh.info.n_audio * o.nch * sizeof(int16_t);
    sh.ar.emplace(lr_bytes, sw.pin_cache);
    sh.rr.emplace(o, spec.rds, spec.rds_clock == SDR_MULTI_RDS_CLOCK_TRACK ? spec.track : nullptr, spec.soft, spec.carrier,
                  sh.info.n_rds, sw.pin_cache);
    if (spec.meter) sh.meter.emplace(o, *spec.meter, sw.pin_cache);
    if (sh.meter && (o.flags & SDR_FLAG_IF_ENVELOPE)) sh.rf.emplace(o, sh.meter->m, sw.pin_cache);
    if (spec.audio) sh.fin.emplace(o, *spec.audio, spec.blend, lr_bytes, sw.pin_cache);
    mark("consumer buffers");
    // two recycled device batches (threadsafequeue.h's one slot, plus the one the producer fills meanwhile)
    for (int i = 0; i < 2; i++) sh.q.add_free(&sh.batches.emplace_back(o.nch, sh.info.block_if).fb);
    check_hip(hipDeviceSynchronize(), "hipDeviceSynchronize");
    mark("batches");
    // one persistent launch per consumer for every block (before the first sdr_push_fm_demod)
    if (sh.persistent) {
        check_sdr(sdr_plls_launch_sel(sh.ctx[1], (int)sh.nblocks_known, SDR_PLLS_STEREO, sh.s_pll[0]), "sdr_plls_launch_sel");
        check_sdr(sdr_plls_launch_sel(sh.ctx[2], (int)sh.nblocks_known, SDR_PLLS_RDS, sh.s_pll[1]), "sdr_plls_launch_sel");
    }
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
    st->blocks = sh.blocks;
    st->seconds = std::chrono::duration<double>(t_end - t0).count();
    st->steady_seconds = sh.blocks >= 2 ? std::chrono::duration<double>(t_end - sh.t_block1).count() : 0.0;
    st->read_s = sh.read_s;
    st->h2d_ms = sh.h2d_ms;
    st->d2h_ms = sh.d2h_ms;
    st->persistent = sh.persistent ? 1 : 0;
    if (sh.persistent) {
        if (sh.blocks != sh.nblocks_known) die("sdr_multi: fewer blocks than the persistent launches cover");
        for (int i = 0; i < 2; i++) {
            double ms[1] = {0.0};
            int nb = 0;
            check_sdr(sdr_plls_report(sh.ctx[1 + i], ms, 0, &nb, sh.s_pll[i]), "sdr_plls_report");   // a timeout fails here
            launch_period_ms(sh.ctx[1 + i], sh.s_pll[i], &st->pll_period_ms, &st->pll_span_ms,
                             o.pll_end ? o.pll_end + (size_t)i * o.stamp_blocks : nullptr, o.stamp_blocks, sw.trace);
        }
    }
    // The one order that matters at the end: the device is idle before sh releases anything, and the
    // splitter's clip counters are read while the splitter exists.
    check_hip(hipDeviceSynchronize(), "hipDeviceSynchronize");
    if (sh.split) check_split(*sh.split, sh.split->report(spec.wide->clips, spec.fmt, nullptr));
    if (sh.meter && o.out_prefix) sh.meter->write_status(std::string(o.out_prefix) + ".status");
    if (sh.rf && o.out_prefix) sh.rf->write_status(std::string(o.out_prefix) + ".rfstatus");
}

int multi_run(const RunSpec& spec, sdr_multi_stats* stats) {
    if (!validate(spec)) return SDR_E_INVALID;
    check_hip(hipSetDevice(spec.o->device), "hipSetDevice");
    const Switches sw{};
    const Trace mark{sw.trace};
    sdr_multi_stats st{};
    run(spec, sw, mark, &st);
    mark("torn down");
    if (stats) *stats = st;
    return SDR_OK;
}

}  // namespace

extern "C" int sdr_multi_run(const sdr_multi_opts* opts, sdr_multi_stats* stats) {
    return multi_run({opts}, stats);
}

extern "C" int sdr_multi_run_tuned(const sdr_multi_opts* opts, const sdr_multi_tuning* tune, sdr_multi_stats* stats) {
    return multi_run({opts, tune}, stats);
}

extern "C" int sdr_multi_run_metered(const sdr_multi_opts* opts, const sdr_multi_tuning* tune, const sdr_meter_opts* mo,
                                     sdr_multi_stats* stats) {
    if (!mo) return SDR_E_INVALID;
    return multi_run({opts, tune, mo}, stats);
}

extern "C" int sdr_multi_run_finished(const sdr_multi_opts* opts, const sdr_multi_tuning* tune, const sdr_meter_opts* mo,
                                      const sdr_audio_opts* ao, int blend, sdr_multi_stats* stats) {
    if (!ao) return SDR_E_INVALID;
    return multi_run({opts, tune, mo, ao, blend != 0}, stats);
}

extern "C" int sdr_multi_run_wide(const sdr_multi_opts* opts, const sdr_multi_wide* wide, const sdr_multi_tuning* tune,
                                  const sdr_meter_opts* mo, const sdr_audio_opts* ao, int blend, sdr_multi_stats* stats) {
    if (!wide) return sdr_multi_run_finished(opts, tune, mo, ao, blend, stats);
    if (!tune) return SDR_E_INVALID;
    return multi_run({opts, tune, mo, ao, blend != 0, wide}, stats);
}

extern "C" int sdr_multi_run_rds(const sdr_multi_opts* opts, const sdr_multi_wide* wide, const sdr_multi_tuning* tune,
                                 const sdr_meter_opts* mo, const sdr_audio_opts* ao, int blend, const sdr_multi_rds* rds,
                                 sdr_multi_stats* stats) {
    if (!rds) return sdr_multi_run_wide(opts, wide, tune, mo, ao, blend, stats);
    if (wide && !tune) return SDR_E_INVALID;
    return multi_run({opts, tune, mo, ao, blend != 0, wide, rds}, stats);
}

extern "C" int sdr_multi_run_rds_clock(const sdr_multi_opts* opts, const sdr_multi_wide* wide, const sdr_multi_tuning* tune,
                                       const sdr_meter_opts* mo, const sdr_audio_opts* ao, int blend, const sdr_multi_rds* rds,
                                       int rds_clock, const sdr_rds_track_opts* track, sdr_multi_stats* stats) {
    return sdr_multi_run_rds_soft(opts, wide, tune, mo, ao, blend, rds, rds_clock, track, nullptr, stats);
}

extern "C" int sdr_multi_run_rds_soft(const sdr_multi_opts* opts, const sdr_multi_wide* wide, const sdr_multi_tuning* tune,
                                      const sdr_meter_opts* mo, const sdr_audio_opts* ao, int blend, const sdr_multi_rds* rds,
                                      int rds_clock, const sdr_rds_track_opts* track, const sdr_rds_soft_opts* soft,
                                      sdr_multi_stats* stats) {
    return sdr_multi_run_rds_carrier(opts, wide, tune, mo, ao, blend, rds, rds_clock, track, soft, nullptr, stats);
}

extern "C" int sdr_multi_run_rds_carrier(const sdr_multi_opts* opts, const sdr_multi_wide* wide, const sdr_multi_tuning* tune,
                                         const sdr_meter_opts* mo, const sdr_audio_opts* ao, int blend, const sdr_multi_rds* rds,
                                         int rds_clock, const sdr_rds_track_opts* track, const sdr_rds_soft_opts* soft,
                                         const sdr_rds_carrier_opts* carrier, sdr_multi_stats* stats) {
    if (rds_clock == SDR_MULTI_RDS_CLOCK_REF) {
        if (soft || carrier) return SDR_E_INVALID;   // the reference clock has no reliabilities and reads rds_clean itself
        return sdr_multi_run_rds(opts, wide, tune, mo, ao, blend, rds, stats);
    }
    if (!rds || (wide && !tune)) return SDR_E_INVALID;
    sdr_rds_track_opts defaults;
    sdr_rds_track_opts_default(&defaults);
    return multi_run({opts, tune, mo, ao, blend != 0, wide, rds, rds_clock, track ? track : &defaults, soft, carrier}, stats);
}

extern "C" int sdr_multi_run_wide_fmt(const sdr_multi_opts* opts, const sdr_multi_wide* wide, const sdr_multi_tuning* tune,
                                      const sdr_meter_opts* mo, const sdr_audio_opts* ao, int blend, const sdr_multi_rds* rds,
                                      int rds_clock, const sdr_rds_track_opts* track, const sdr_rds_soft_opts* soft,
                                      const sdr_rds_carrier_opts* carrier, const sdr_wide_fmt* fmt, sdr_multi_stats* stats) {
    if (!sdrhost::wide16(fmt))
        return sdr_multi_run_rds_carrier(opts, wide, tune, mo, ao, blend, rds, rds_clock, track, soft, carrier, stats);
    if (!wide || !tune) return SDR_E_INVALID;   // int16 rows are wide rows, and a wide run is always tuned
    // the chain of entry points below this one, with the record: each step's own refusals, then the run
    if (rds_clock == SDR_MULTI_RDS_CLOCK_REF) {
        if (soft || carrier) return SDR_E_INVALID;
        return multi_run({opts, tune, mo, ao, blend != 0, wide, rds, SDR_MULTI_RDS_CLOCK_REF, nullptr, nullptr, nullptr, fmt}, stats);
    }
    if (!rds) return SDR_E_INVALID;
    sdr_rds_track_opts defaults;
    sdr_rds_track_opts_default(&defaults);
    return multi_run({opts, tune, mo, ao, blend != 0, wide, rds, rds_clock, track ? track : &defaults, soft, carrier, fmt}, stats);
}
