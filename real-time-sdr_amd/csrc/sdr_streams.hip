// sdr_streams.hip -- what the library keeps per stream rather than per context: the CU-masked
// streams of sdr_stream_create_cu_range with their placement, the per-stream scratch of sdr_fmpll,
// the bandwidth calibration copy sdr_hbm_copy, and the test and diagnosis hooks (sdr_diag_*).

#include "sdr_internal.h"

#include <algorithm>
#include <mutex>
#include <vector>

#pragma clang fp contract(off)

using namespace sdrk;

namespace {

// Scratch of the context-free PLL primitive (input reciprocals [nch][ts] f64 + phases [nch][ts]
// f32): one buffer per (device, stream), reused in that stream's order and grown on demand, so
// sdr_fmpll enqueues without synchronising (the round-2 diagnosis of the pool-allocated variants
// that this replaced: DESIGN.md 7, profiles/r02/diag_fmpll_scratch.txt).
struct StreamScratch {
    hipStream_t s;
    int dev;
    void* p;
    size_t bytes;
};
std::vector<StreamScratch> g_scratch;

// forget (and free) the scratch of a stream about to be destroyed
int release_stream_scratch(hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    for (size_t i = 0; i < g_scratch.size(); i++) {
        if (g_scratch[i].s != s) continue;
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipFree(g_scratch[i].p));
        g_scratch.erase(g_scratch.begin() + (long)i);
        return SDR_OK;
    }
    return SDR_OK;
}

// Streams made by sdr_stream_create_cu_range, with their device, CU mask and placement. The
// persistent PLL launch accepts only these: each has its own hardware queue (a pool stream can share
// one with the stream that signals the blocks, which then never runs), and its mask's placement
// bounds how many of the launch's workgroups can be resident at once (sdr_internal.h CuPlacement).
struct MaskedStream {
    hipStream_t s;
    int device;
    CuPlacement place;
};
std::mutex g_masked_mu;
std::vector<MaskedStream> g_masked;

// Bandwidth calibration (sdr_hbm_copy): one 16-byte element per lane, one short-lived workgroup per
// 4 KiB -- the fastest plain copy measured on this device (tools/hbm_copy_bench.hip: 6.2 TB/s, where
// grid-stride loops with 1-8 loads in flight per lane reach 4.1-5.7) -- the HBM rate a plain stream
// reaches, the practical ceiling the front end's roofline fraction is read against.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_hbm_copy(u32x4* __restrict__ dst, const u32x4* __restrict__ src, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

}  // namespace

namespace sdrk {

std::mutex g_scratch_mu;

int stream_scratch(hipStream_t s, size_t bytes, void** out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    for (auto& e : g_scratch) {
        if (e.s != s || e.dev != dev) continue;
        if (e.bytes < bytes) {   // grow: work already queued on s may still read the old buffer
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(hipFree(e.p));
            e.p = nullptr;
            HIP_TRY(hipMalloc(&e.p, bytes));
            e.bytes = bytes;
        }
        *out = e.p;
        return SDR_OK;
    }
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    g_scratch.push_back({s, dev, p, bytes});
    *out = p;
    return SDR_OK;
}

bool masked_stream(hipStream_t s, int* device, CuPlacement* place) {
    std::lock_guard<std::mutex> lk(g_masked_mu);
    for (const MaskedStream& m : g_masked)
        if (m.s == s && s != nullptr) {
            *device = m.device;
            if (place) *place = m.place;
            return true;
        }
    return false;
}

std::vector<uint32_t> cu_range_mask(int ncu, int first_cu, int n_cu, int exclude, int* nset) {
    std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
    *nset = 0;
    for (int cu = 0; cu < ncu; ++cu) {
        const bool in = cu >= first_cu && cu < first_cu + n_cu;
        if (in != (exclude != 0)) {
            mask[cu / 32] |= 1u << (cu % 32);
            ++*nset;
        }
    }
    return mask;
}

int device_xccs(int device) {
    int nx = 0;
    if (hipDeviceGetAttribute(&nx, hipDeviceAttributeNumberOfXccs, device) != hipSuccess || nx <= 0) nx = 8;
    return nx;
}

}  // namespace sdrk

CuPlacement sdrk::cu_placement(const uint32_t* mask, int nwords, int ncu_dev, int nxcc) {
    constexpr int SE_PER_XCC = 4;   // MI355X: 32 shader engines over 8 XCCs
    CuPlacement pl;
    if (nxcc <= 0 || ncu_dev % nxcc) nxcc = 1;
    const int slots = ncu_dev / nxcc;
    int min_units = -1;
    for (int x = 0; x < nxcc; x++) {
        int per_se[SE_PER_XCC] = {};
        int nx = 0;
        for (int j = 0; j < slots; j++) {
            const int bit = j * nxcc + x;
            if (bit / 32 < nwords && (mask[bit / 32] >> (bit % 32) & 1u)) {
                per_se[j % SE_PER_XCC]++;
                nx++;
            }
        }
        pl.ncu += nx;
        if (!nx) continue;
        pl.xcc_active++;
        int active = 0, lo = slots;
        for (int k = 0; k < SE_PER_XCC; k++)
            if (per_se[k]) {
                active++;
                lo = std::min(lo, per_se[k]);
            }
        const int units = active * lo;
        min_units = min_units < 0 ? units : std::min(min_units, units);
    }
    pl.min_units = std::max(min_units, 0);
    return pl;
}

extern "C" {

int sdr_stream_create_cu_range(void** stream, int device, int first_cu, int n_cu, int exclude) {
    if (!stream) return fail(SDR_E_INVALID, "sdr_stream_create_cu_range: stream is NULL");
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    struct Restore {   // the caller's current device is left as it was
        int d;
        ~Restore() { (void)hipSetDevice(d); }
    } restore{cur};
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    const int ncu = prop.multiProcessorCount;
    if (first_cu < 0 || n_cu <= 0 || first_cu + n_cu > ncu || (exclude && n_cu >= ncu))
        return fail(SDR_E_INVALID, "sdr_stream_create_cu_range: CUs [%d, %d) outside [0, %d)",
                    first_cu, first_cu + n_cu, ncu);
    int nset = 0;
    std::vector<uint32_t> mask = cu_range_mask(ncu, first_cu, n_cu, exclude, &nset);
    hipStream_t s = nullptr;
    HIP_TRY(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
    {
        std::lock_guard<std::mutex> lk(g_masked_mu);
        g_masked.push_back(MaskedStream{s, device, cu_placement(mask.data(), (int)mask.size(), ncu, device_xccs(device))});
    }
    *stream = s;
    return SDR_OK;
}

int sdr_stream_destroy(void* stream) {
    if (!stream) return fail(SDR_E_INVALID, "sdr_stream_destroy: stream is NULL");
    const int rc = release_stream_scratch((hipStream_t)stream);
    if (rc != SDR_OK) return rc;
    {
        std::lock_guard<std::mutex> lk(g_masked_mu);
        for (size_t i = 0; i < g_masked.size(); i++)
            if (g_masked[i].s == (hipStream_t)stream) {
                g_masked.erase(g_masked.begin() + (long)i);
                break;
            }
    }
    HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return SDR_OK;
}

int sdr_hbm_copy(void* dst, const void* src, size_t bytes, void* stream) {
    if (!dst || !src || (bytes & 15) || (reinterpret_cast<uintptr_t>(dst) & 15) || (reinterpret_cast<uintptr_t>(src) & 15))
        return fail(SDR_E_INVALID, "sdr_hbm_copy: pointers and size must be 16-byte aligned");
    if (bytes == 0) return SDR_OK;
    const size_t n = bytes / 16;
    if ((n + 255) / 256 > 0x7FFFFFFFu) return fail(SDR_E_INVALID, "sdr_hbm_copy: %zu bytes is too large", bytes);
    const int grid = (int)((n + 255) / 256);
    hipLaunchKernelGGL(k_hbm_copy, dim3(grid), dim3(256), 0, S(stream), static_cast<u32x4*>(dst),
                       static_cast<const u32x4*>(src), n);
    HIP_TRY(hipGetLastError());
    return SDR_OK;
}

// Test support (not part of sdr_amd.h): hold `stream` for `ms` milliseconds (at most 10 s) with one
// sleeping wave, so that a test can keep a reader stream from releasing its block (the bounded
// release wait's timeout, tests/test_gpu_pipeline.py). (The two test kernels have C linkage, the
// names k_hold and k_rcp64_residual, in profiles and traces.)
__global__ void k_hold(unsigned long long ticks) {
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}
int sdr_diag_hold(void* stream, int ms) {
    if (ms < 0 || ms > 10000) return fail(SDR_E_INVALID, "sdr_diag_hold: %d ms outside [0, 10000]", ms);
    hipLaunchKernelGGL(k_hold, dim3(1), dim3(64), 0, S(stream), (unsigned long long)ms * 100000ull);
    HIP_TRY(hipGetLastError());
    return SDR_OK;
}

// Test support (not part of sdr_amd.h): res[i] = 1 - x[i] * v_rcp_f64(x[i]) (one fma, exact), the
// hardware reciprocal's relative error that the exact front end's discriminator proof assumes
// below 2^-22 (sdr_frontend.hip, SDR_FE_DISC; tests/test_gpu_primitives.py).
__global__ void k_rcp64_residual(const double* __restrict__ x, double* __restrict__ res, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) res[i] = __builtin_fma(-x[i], __builtin_amdgcn_rcp(x[i]), 1.0);
}
int sdr_diag_rcp64_residual(const double* x, double* res, int n, void* stream) {
    if (!x || !res || n <= 0) return fail(SDR_E_INVALID, "sdr_diag_rcp64_residual: bad arguments");
    hipLaunchKernelGGL(k_rcp64_residual, dim3((n + 255) / 256), dim3(256), 0, S(stream), x, res, n);
    HIP_TRY(hipGetLastError());
    return SDR_OK;
}

// Diagnosis builds only (-DSDR_PLL_COUNT=1): the PLL chunk counters; -1 in product builds.
// Not part of sdr_amd.h.
int sdr_diag_pll_counts(unsigned long long* out, int reset) { return diag_pll_counts(out, reset); }
// Diagnosis builds only (-DSDR_PLL_WAVES=1): per-wave totals of the last persistent launch; -1 otherwise.
int sdr_diag_pll_waves(unsigned long long* out, int nmax) { return diag_pll_waves(out, nmax); }
// Diagnosis builds only (-DSDR_PLL_HWID=1): placement and duration of the last k_pll launch's waves.
int sdr_diag_pll_hwid(unsigned long long* out, int nmax) { return diag_pll_hwid(out, nmax); }

}  // extern "C"
