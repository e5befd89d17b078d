// sdr_scan_run.cpp -- the band scans over a capture file, one loop for both: read blocks, sdr_scan_block
// each, pick every row's stations, write the --tune list.
//   sdr_scan_run (include/sdr_scan_run.h): the blocks hold capture rows; list entry src is the row.
//   sdr_wide_scan_run (include/sdr_wide_scan.h): the blocks hold wide streams, which sdr_split_block cuts
//     into capture rows in front of the scanner; every row is picked on the absolute station grid.
//   sdr_wide_scan_run_fmt (include/sdr_multi_wide16.h): the same on int16 wide streams (sdr_split16_block), with a
//     shift per row, fixed or taken from block 0's peaks before the scan starts at block 0.
// The plain scan is the wide one without a splitter: one row per input stream, the caller's pick options.
#include "sdr_scan_run.h"
#include "sdr_wide_scan.h"
#include "sdr_multi_wide16.h"
#include "wide_split.h"

#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <set>
#include <vector>

namespace {
int fail(sdr_wide_scan_stats* st, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(st->error, sizeof(st->error), fmt, ap);
    va_end(ap);
    return code;
}

// everything the run holds, released on every way out
struct Run {
    FILE* in = nullptr;
    bool close_in = false;
    sdrhost::WideSplit split;                     // a wide scan's
    sdr_scan* scan = nullptr;
    uint8_t *d_in = nullptr, *d_rows = nullptr;   // the uploaded block; a wide scan's capture rows
    hipStream_t stream = nullptr;
    ~Run() {
        if (scan) sdr_scan_destroy(scan);
        split.close();
        if (d_in) (void)hipFree(d_in);
        if (d_rows) (void)hipFree(d_rows);
        if (stream) (void)hipStreamDestroy(stream);
        if (in && close_in) std::fclose(in);
    }
};

// o->nwide input streams per block; wide: each is a wide stream of o->W, else a capture row (W, shift unused)
// fmt (a wide scan's only): int16 wide streams
int scan_file(const sdr_wide_scan_opts* o, bool wide, sdr_wide_scan_stats* st, const sdr_wide_fmt* fmt = nullptr) {
    const bool s16 = sdrhost::wide16(fmt);
    const char* who = wide ? "wide scan" : "scan";
    std::memset(st, 0, sizeof(*st));
    if (!o || !o->in_path || o->nwide < 1)
        return fail(st, SDR_E_INVALID, "%s: needs an input and %s >= 1", who, wide ? "nwide" : "nrows");
    if (o->max_stations > 0 && (!o->src || !o->khz)) return fail(st, SDR_E_INVALID, "%s: null station arrays", who);
    // (the plain scan leaves the step to sdr_scan_pick, after the blocks)
    if (wide && o->pick.step_khz < 1) return fail(st, SDR_E_INVALID, "%s: step < 1", who);
    int R = 1, in_iq = 0, half = 0, N = 0, block_iq = 0;
    if ((wide && sdr_split_geometry(o->mode, o->W, &R, nullptr, &in_iq, &half, nullptr) != SDR_OK) ||
        sdr_scan_geometry(o->mode, &N, nullptr, &block_iq) != SDR_OK)
        return fail(st, SDR_E_INVALID, "%s: %s", who, sdr_last_error());
    if (!wide) in_iq = block_iq;
    if (s16)
        if (const char* why = sdrhost::wide_fmt_refusal(fmt, o->mode, o->W, o->nwide, o->shift))
            return fail(st, SDR_E_INVALID, "%s: %s", who, why);
    const int max_blocks = o->max_blocks > 0 ? o->max_blocks : 4;
    const int nrows = o->nwide * R;
    Run r;
    if (std::strcmp(o->in_path, "-") == 0) {
        r.in = stdin;
    } else {
        r.in = std::fopen(o->in_path, "rb");
        r.close_in = true;
    }
    if (!r.in) return fail(st, SDR_E_INVALID, "%s: cannot open %s", who, o->in_path);
    const size_t in_bytes = (size_t)(s16 ? 4 : 2) * in_iq, block_bytes = in_bytes * (size_t)o->nwide;
    const size_t row_bytes = (size_t)2 * block_iq;
    int rc = wide ? r.split.create(o->device, o->mode, o->W, o->nwide, o->shift, fmt) : SDR_OK;
    if (rc == SDR_OK) rc = sdr_scan_create(&r.scan, o->device, o->mode, nrows);
    if (rc != SDR_OK) return fail(st, rc, "%s: %s", who, sdr_last_error());
    if (hipSetDevice(o->device) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&r.d_in), block_bytes) != hipSuccess ||
        (wide && hipMalloc(reinterpret_cast<void**>(&r.d_rows), row_bytes * (size_t)nrows) != hipSuccess) ||
        hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking) != hipSuccess) {
        if (wide)
            return fail(st, SDR_E_HIP, "wide scan: no device buffers of %zu and %zu bytes or no stream", block_bytes,
                        row_bytes * (size_t)nrows);
        return fail(st, SDR_E_HIP, "scan: no device buffer of %zu bytes or no stream", block_bytes);
    }
    if (wide && r.split.set_table(fmt, r.stream) != SDR_OK) return fail(st, SDR_E_INVALID, "%s: %s", who, sdr_last_error());
    std::vector<uint8_t> host(block_bytes);
    while (st->blocks < max_blocks && std::fread(host.data(), 1, block_bytes, r.in) == block_bytes) {
        // (the copy returns once the pageable buffer is staged; the kernels of the previous block read
        // d_in and d_rows in stream order before it)
        if (hipMemcpyAsync(r.d_in, host.data(), block_bytes, hipMemcpyHostToDevice, r.stream) != hipSuccess ||
            hipStreamSynchronize(r.stream) != hipSuccess)
            return fail(st, SDR_E_HIP, "%s: upload of block %lld failed", who, st->blocks);
        if (wide && st->blocks == 0 && r.split.auto_target >= 0)   // (d_rows is written again below)
            rc = r.split.gain_from(r.d_in, in_bytes, r.d_rows, row_bytes, r.stream);
        if (wide && rc == SDR_OK) rc = r.split.block(r.d_in, in_bytes, r.d_rows, row_bytes, r.stream);
        if (rc == SDR_OK) rc = sdr_scan_block(r.scan, wide ? r.d_rows : r.d_in, row_bytes, r.stream);
        if (rc != SDR_OK) return fail(st, rc, "%s: %s", who, sdr_last_error());
        st->blocks++;
    }
    if (st->blocks == 0)
        return fail(st, SDR_E_INVALID, "%s: %s holds no whole block of %d %s (%zu bytes)", who, o->in_path, o->nwide,
                    wide ? "wide streams" : "rows", block_bytes);
    std::vector<float> psd((size_t)nrows * N);
    rc = sdr_scan_psd(r.scan, psd.data(), &st->segments, r.stream);
    std::vector<long long> clips((size_t)nrows);
    if (rc == SDR_OK && wide) rc = r.split.report(clips.data(), fmt, r.stream);
    if (rc != SDR_OK) return fail(st, rc, "%s: %s", who, sdr_last_error());
    for (long long c : clips) st->clips += c;
    std::vector<int32_t> src, khz, row_khz(N + 1);
    std::vector<float> row_db(N + 1);
    const long long step = o->pick.step_khz;
    for (int w = 0; w < o->nwide; w++) {
        std::set<long long> seen;                      // absolute kHz already given by an earlier row of this wide stream
        for (int row = 0; row < R; row++) {
            sdr_scan_opts p = o->pick;
            long long centre = 0;
            if (wide) {
                centre = (long long)(row - (o->W - 1)) * half;
                p.guard_khz = N / 4;
                p.first_khz = (int)((((long long)o->pick.first_khz - centre) % step + step) % step);
            }
            int n = 0;
            rc = sdr_scan_pick(o->mode, psd.data() + ((size_t)w * R + row) * N, &p, row_khz.data(), row_db.data(), N + 1, &n);
            if (rc != SDR_OK) return fail(st, rc, "%s: %s", who, sdr_last_error());
            for (int i = 0; i < n && i <= N; i++)
                if (!wide || seen.insert(centre + row_khz[i]).second) {
                    src.push_back(w * R + row);
                    khz.push_back(row_khz[i]);
                }
        }
    }
    st->stations = (int)src.size();
    for (int i = 0; i < o->max_stations && i < st->stations; i++) {
        o->src[i] = src[i];
        o->khz[i] = khz[i];
    }
    if (o->out_path) {
        FILE* f = std::fopen(o->out_path, "w");
        if (!f) return fail(st, SDR_E_INVALID, "%s: cannot write %s", who, o->out_path);
        for (size_t i = 0; i < src.size(); i++) std::fprintf(f, "%d %d\n", (int)src[i], (int)khz[i]);
        if (std::fclose(f) != 0) return fail(st, SDR_E_INVALID, "%s: cannot write %s", who, o->out_path);
    }
    return SDR_OK;
}
}  // namespace

extern "C" int sdr_wide_scan_run(const sdr_wide_scan_opts* o, sdr_wide_scan_stats* st) {
    return st ? scan_file(o, true, st) : SDR_E_INVALID;
}

extern "C" int sdr_wide_scan_run_fmt(const sdr_wide_scan_opts* o, const sdr_wide_fmt* fmt, sdr_wide_scan_stats* st) {
    return st ? scan_file(o, true, st, fmt) : SDR_E_INVALID;
}

extern "C" int sdr_scan_run(const sdr_scan_run_opts* o, sdr_scan_run_stats* st) {
    if (!st) return SDR_E_INVALID;
    sdr_wide_scan_opts w{};
    if (o) {
        w.nwide = o->nrows;
        w.mode = o->mode;
        w.device = o->device;
        w.in_path = o->in_path;
        w.out_path = o->out_path;
        w.max_blocks = o->max_blocks;
        w.pick = o->pick;
        w.max_stations = o->max_stations;
        w.src = o->src;
        w.khz = o->khz;
    }
    sdr_wide_scan_stats ws;
    const int rc = scan_file(o ? &w : nullptr, false, &ws);
    st->stations = ws.stations;
    st->blocks = ws.blocks;
    st->segments = ws.segments;
    std::memcpy(st->error, ws.error, sizeof(st->error));
    return rc;
}
