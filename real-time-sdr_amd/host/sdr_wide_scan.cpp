// sdr_wide_scan.cpp -- the band scan over a wide capture file (include/sdr_wide_scan.h): read wide
// blocks, sdr_split_block each into capture rows, sdr_scan_block the rows, pick every row's stations on
// the absolute grid, write the --tune list.
#include "sdr_wide_scan.h"

#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstdio>
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
    sdr_split* split = nullptr;
    sdr_scan* scan = nullptr;
    int8_t* d_wide = nullptr;
    uint8_t* d_rows = nullptr;
    hipStream_t stream = nullptr;
    ~Run() {
        if (scan) sdr_scan_destroy(scan);
        if (split) sdr_split_destroy(split);
        if (d_wide) (void)hipFree(d_wide);
        if (d_rows) (void)hipFree(d_rows);
        if (stream) (void)hipStreamDestroy(stream);
        if (in && close_in) std::fclose(in);
    }
};
}  // namespace

extern "C" int sdr_wide_scan_run(const sdr_wide_scan_opts* o, sdr_wide_scan_stats* st) {
    if (!st) return SDR_E_INVALID;
    std::memset(st, 0, sizeof(*st));
    if (!o || !o->in_path || o->nwide < 1) return fail(st, SDR_E_INVALID, "wide scan: needs an input and nwide >= 1");
    if (o->max_stations > 0 && (!o->src || !o->khz)) return fail(st, SDR_E_INVALID, "wide scan: null station arrays");
    if (o->pick.step_khz < 1) return fail(st, SDR_E_INVALID, "wide scan: step < 1");
    int R = 0, wide_iq = 0, half = 0, N = 0, seg = 0, block_iq = 0;
    if (sdr_split_geometry(o->mode, o->W, &R, nullptr, &wide_iq, &half, nullptr) != SDR_OK ||
        sdr_scan_geometry(o->mode, &N, &seg, &block_iq) != SDR_OK)
        return fail(st, SDR_E_INVALID, "wide scan: %s", sdr_last_error());
    const int max_blocks = o->max_blocks > 0 ? o->max_blocks : 4;
    const int nrows = o->nwide * R;
    Run r;
    if (std::strcmp(o->in_path, "-") == 0) {
        r.in = stdin;
    } else {
        r.in = std::fopen(o->in_path, "rb");
        r.close_in = true;
    }
    if (!r.in) return fail(st, SDR_E_INVALID, "wide scan: cannot open %s", o->in_path);
    const size_t wide_bytes = (size_t)2 * wide_iq, block_bytes = wide_bytes * (size_t)o->nwide;
    const size_t row_bytes = (size_t)2 * block_iq;
    int rc = sdr_split_create(&r.split, o->device, o->mode, o->W, o->nwide, o->shift);
    if (rc == SDR_OK) rc = sdr_scan_create(&r.scan, o->device, o->mode, nrows);
    if (rc != SDR_OK) return fail(st, rc, "wide scan: %s", sdr_last_error());
    if (hipSetDevice(o->device) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&r.d_wide), block_bytes) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&r.d_rows), row_bytes * (size_t)nrows) != hipSuccess ||
        hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking) != hipSuccess)
        return fail(st, SDR_E_HIP, "wide scan: no device buffers of %zu and %zu bytes or no stream", block_bytes,
                    row_bytes * (size_t)nrows);
    std::vector<int8_t> host(block_bytes);
    while (st->blocks < max_blocks && std::fread(host.data(), 1, block_bytes, r.in) == block_bytes) {
        // (the copy returns once the pageable buffer is staged; the kernels of the previous block read
        // d_wide and d_rows in stream order before it)
        if (hipMemcpyAsync(r.d_wide, host.data(), block_bytes, hipMemcpyHostToDevice, r.stream) != hipSuccess ||
            hipStreamSynchronize(r.stream) != hipSuccess)
            return fail(st, SDR_E_HIP, "wide scan: upload of block %lld failed", st->blocks);
        rc = sdr_split_block(r.split, r.d_wide, wide_bytes, r.d_rows, row_bytes, r.stream);
        if (rc == SDR_OK) rc = sdr_scan_block(r.scan, r.d_rows, row_bytes, r.stream);
        if (rc != SDR_OK) return fail(st, rc, "wide scan: %s", sdr_last_error());
        st->blocks++;
    }
    if (st->blocks == 0)
        return fail(st, SDR_E_INVALID, "wide scan: %s holds no whole block of %d wide streams (%zu bytes)", o->in_path,
                    o->nwide, block_bytes);
    std::vector<float> psd((size_t)nrows * N);
    rc = sdr_scan_psd(r.scan, psd.data(), &st->segments, r.stream);
    std::vector<long long> clips((size_t)nrows);
    if (rc == SDR_OK) rc = sdr_split_clips(r.split, clips.data(), r.stream);
    if (rc != SDR_OK) return fail(st, rc, "wide scan: %s", sdr_last_error());
    for (long long c : clips) st->clips += c;
    std::vector<int32_t> src, khz, row_khz(N + 1);
    std::vector<float> row_db(N + 1);
    const long long step = o->pick.step_khz;
    for (int w = 0; w < o->nwide; w++) {
        std::set<long long> seen;                      // absolute kHz already given by an earlier row of this stream
        for (int row = 0; row < R; row++) {
            const long long centre = (long long)(row - (o->W - 1)) * half;
            sdr_scan_opts p = o->pick;
            p.guard_khz = N / 4;
            p.first_khz = (int)((((long long)o->pick.first_khz - centre) % step + step) % step);
            int n = 0;
            rc = sdr_scan_pick(o->mode, psd.data() + ((size_t)w * R + row) * N, &p, row_khz.data(), row_db.data(), N + 1, &n);
            if (rc != SDR_OK) return fail(st, rc, "wide scan: %s", sdr_last_error());
            for (int i = 0; i < n && i <= N; i++)
                if (seen.insert(centre + row_khz[i]).second) {
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
        if (!f) return fail(st, SDR_E_INVALID, "wide scan: cannot write %s", o->out_path);
        for (size_t i = 0; i < src.size(); i++) std::fprintf(f, "%d %d\n", (int)src[i], (int)khz[i]);
        if (std::fclose(f) != 0) return fail(st, SDR_E_INVALID, "wide scan: cannot write %s", o->out_path);
    }
    return SDR_OK;
}
