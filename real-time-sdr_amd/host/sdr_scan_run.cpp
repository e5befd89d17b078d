// sdr_scan_run.cpp -- the band scan over a capture file (include/sdr_scan_run.h): read blocks of
// capture rows, sdr_scan_block each, pick every row's stations, write the --tune list.
#include "sdr_scan_run.h"

#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {
int fail(sdr_scan_run_stats* st, int code, const char* fmt, ...) {
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
    sdr_scan* scan = nullptr;
    uint8_t* d_iq = nullptr;
    hipStream_t stream = nullptr;
    ~Run() {
        if (scan) sdr_scan_destroy(scan);
        if (d_iq) (void)hipFree(d_iq);
        if (stream) (void)hipStreamDestroy(stream);
        if (in && close_in) std::fclose(in);
    }
};
}  // namespace

extern "C" int sdr_scan_run(const sdr_scan_run_opts* o, sdr_scan_run_stats* st) {
    if (!st) return SDR_E_INVALID;
    std::memset(st, 0, sizeof(*st));
    if (!o || !o->in_path || o->nrows < 1) return fail(st, SDR_E_INVALID, "scan: needs an input and nrows >= 1");
    if (o->max_stations > 0 && (!o->src || !o->khz)) return fail(st, SDR_E_INVALID, "scan: null station arrays");
    int N = 0, seg = 0, block_iq = 0;
    if (sdr_scan_geometry(o->mode, &N, &seg, &block_iq) != SDR_OK) return fail(st, SDR_E_INVALID, "scan: %s", sdr_last_error());
    const int max_blocks = o->max_blocks > 0 ? o->max_blocks : 4;
    Run r;
    if (std::strcmp(o->in_path, "-") == 0) {
        r.in = stdin;
    } else {
        r.in = std::fopen(o->in_path, "rb");
        r.close_in = true;
    }
    if (!r.in) return fail(st, SDR_E_INVALID, "scan: cannot open %s", o->in_path);
    const size_t row_bytes = (size_t)2 * block_iq, block_bytes = row_bytes * (size_t)o->nrows;
    int rc = sdr_scan_create(&r.scan, o->device, o->mode, o->nrows);
    if (rc != SDR_OK) return fail(st, rc, "scan: %s", sdr_last_error());
    if (hipSetDevice(o->device) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&r.d_iq), block_bytes) != hipSuccess ||
        hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking) != hipSuccess)
        return fail(st, SDR_E_HIP, "scan: no device buffer of %zu bytes or no stream", block_bytes);
    std::vector<uint8_t> host(block_bytes);
    while (st->blocks < max_blocks && std::fread(host.data(), 1, block_bytes, r.in) == block_bytes) {
        // (the copy returns once the pageable buffer is staged; the kernels of the previous block
        // read d_iq in stream order before it)
        if (hipMemcpyAsync(r.d_iq, host.data(), block_bytes, hipMemcpyHostToDevice, r.stream) != hipSuccess ||
            hipStreamSynchronize(r.stream) != hipSuccess)
            return fail(st, SDR_E_HIP, "scan: upload of block %lld failed", st->blocks);
        rc = sdr_scan_block(r.scan, r.d_iq, row_bytes, r.stream);
        if (rc != SDR_OK) return fail(st, rc, "scan: %s", sdr_last_error());
        st->blocks++;
    }
    if (st->blocks == 0) return fail(st, SDR_E_INVALID, "scan: %s holds no whole block of %d rows (%zu bytes)", o->in_path, o->nrows, block_bytes);
    std::vector<float> psd((size_t)o->nrows * N);
    rc = sdr_scan_psd(r.scan, psd.data(), &st->segments, r.stream);
    if (rc != SDR_OK) return fail(st, rc, "scan: %s", sdr_last_error());
    std::vector<int32_t> src, khz, row_khz(N + 1);
    std::vector<float> row_db(N + 1);
    for (int row = 0; row < o->nrows; row++) {
        int n = 0;
        rc = sdr_scan_pick(o->mode, psd.data() + (size_t)row * N, &o->pick, row_khz.data(), row_db.data(), N + 1, &n);
        if (rc != SDR_OK) return fail(st, rc, "scan: %s", sdr_last_error());
        for (int i = 0; i < n && i <= N; i++) {
            src.push_back(row);
            khz.push_back(row_khz[i]);
        }
    }
    st->stations = (int)src.size();
    for (int i = 0; i < o->max_stations && i < st->stations; i++) {
        o->src[i] = src[i];
        o->khz[i] = khz[i];
    }
    if (o->out_path) {
        FILE* f = std::fopen(o->out_path, "w");
        if (!f) return fail(st, SDR_E_INVALID, "scan: cannot write %s", o->out_path);
        for (size_t i = 0; i < src.size(); i++) std::fprintf(f, "%d %d\n", (int)src[i], (int)khz[i]);
        if (std::fclose(f) != 0) return fail(st, SDR_E_INVALID, "scan: cannot write %s", o->out_path);
    }
    return SDR_OK;
}
