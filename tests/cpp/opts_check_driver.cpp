// opts_check_driver.cpp -- every sdr_*_check function of libsdr_amd.so (include/sdr_amd.h) over the grid of
// tests/test_opts_check.py, and a NULL for each pointer argument; the 16-bit splitter's gain rule at its ends; and
// the splitters' tap table (sdr_split_taps) and, through the creates on a device that does not exist, the tap
// fragments and column sums built from it: a stand-alone program for a sanitizer run of
// the library's host code. The checks are host arithmetic, so it runs on a machine without a GPU. Build it with
// the library's translation units, all with the sanitizer on the host side only, and run it:
//   for f in real-time-sdr_amd/csrc/*.hip real-time-sdr_amd/csrc/*.cpp tests/cpp/opts_check_driver.cpp; do
//     hipcc $HIPFLAGS -Xarch_host -fsanitize=address,undefined -c -o $OBJ/$(basename $f).o $f; done   # the Makefile's
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o opts_check_driver $OBJ/*.o && ./opts_check_driver
// (objects only on the link line: hipcc reads whatever stands beside a .cpp there as HIP source)
// Prints the number of points accepted and refused; exits 1 when a verdict is not the documented one.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>
#include <vector>

#include "sdr_amd.h"

static int accepted = 0, refused = 0, wrong = 0;

static void expect(int rc, bool legal, const char* what, int mode) {
    (rc == SDR_OK ? accepted : refused)++;
    if ((rc == SDR_OK) != legal || (rc != SDR_OK && (rc != SDR_E_INVALID || !sdr_last_error()[0]))) {
        std::printf("WRONG %s (mode %d): rc %d, \"%s\"\n", what, mode, rc, sdr_last_error());
        wrong++;
    }
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (int mb : {-1, 0, 2, 5, 6})
        for (int lb : {0, 1, 8, 64, 65}) {
            const bool ok = mb >= 0 && mb <= 5 && lb >= 1 && lb <= 64;
            const sdr_rds_opts o{mb, lb};
            expect(sdr_rds_opts_check(&o), ok, "rds_opts", 0);
            for (int sb : {-1, 0, 6, 7}) {
                const sdr_rds_soft_opts s{mb, lb, sb};
                expect(sdr_rds_soft_opts_check(&s), ok && sb >= 0 && sb <= 6, "rds_soft_opts", 0);
            }
        }
    expect(sdr_rds_opts_check(nullptr), false, "rds_opts NULL", 0);
    expect(sdr_rds_soft_opts_check(nullptr), false, "rds_soft_opts NULL", 0);
    for (int mode = -1; mode <= 4; mode++) {
        for (int q : {-1, 0, 10, 15, 16}) {
            const bool qok = mode == 0 && q >= 0 && q <= 15;
            for (int a : {0, 1, 32, 64, 65})
                for (int hb : {15, 16, 40, 64, 65, 80}) {
                    const sdr_rds_track_opts t{q, a, hb};
                    expect(sdr_rds_track_opts_check(mode, &t), qok && a >= 1 && a <= 64 && hb >= 16 && hb <= 64 && hb % 16 == 0,
                           "rds_track_opts", mode);
                }
            for (int av : {-1, 0, 3, 6, 7}) {
                const sdr_rds_carrier_opts c{q, av};
                expect(sdr_rds_carrier_opts_check(mode, &c), qok && av >= 0 && av <= 6, "rds_carrier_opts", mode);
            }
        }
        expect(sdr_rds_track_opts_check(mode, nullptr), false, "rds_track_opts NULL", mode);
        expect(sdr_rds_carrier_opts_check(mode, nullptr), false, "rds_carrier_opts NULL", mode);
        const bool mok = mode >= 0 && mode <= 3;
        for (float tau : {-0.5f, 0.0f, 75.0f, 1000.0f, 1000.5f, nan})
            for (float lo : {-inf, -1.0f, 0.5f, 1.999f, 2.0f, nan})
                for (float hi : {0.5f, 0.501f, 2.0f, 1e30f, inf, nan}) {
                    const sdr_audio_opts a{tau, lo, hi};
                    expect(sdr_audio_opts_check(mode, &a),
                           mok && tau >= 0.0f && tau <= 1000.0f && std::isfinite(lo) && std::isfinite(hi) && hi > lo, "audio_opts",
                           mode);
                }
        expect(sdr_audio_opts_check(mode, nullptr), false, "audio_opts NULL", mode);
        for (int W : {3, 4, 5, 8, 10, 11})
            for (int nw : {0, 1, 4096, 4097})
                for (int sh : {-1, 0, 1, 13, 24, 25})
                    expect(sdr_split_check(mode, W, nw, sh), mok && (W == 4 || W == 8 || W == 10) && nw >= 1 && nw <= 4096 && sh <= 24,
                           "split", mode);
        for (int W : {3, 4, 5, 8, 10, 11})
            for (int nw : {0, 1, 4096, 4097})
                for (int sh : {-1, 0, 1, 22, 33, 34})
                    expect(sdr_split16_check(mode, W, nw, sh), mok && (W == 4 || W == 8 || W == 10) && nw >= 1 && nw <= 4096 && sh <= 33,
                           "split16", mode);
        const int half = mode == 0 || mode == 2 ? 1200 : mode == 1 ? 720 : mode == 3 ? 576 : 0;   // rf_Fs / 2000
        constexpr int NCH = 3;
        for (int nsrc : {-1, 0, 1, 2, NCH, NCH + 1})
            for (int s : {-1, 0, 1, 2, 3})
                for (int k : {-half - 1, -half, -half + 1, 0, half, half + 1, 1 << 30, -(1 << 30)})
                    for (int at = 0; at < NCH; at++) {   // the one channel that is off; the last one included
                        int32_t src[NCH] = {0, 0, 0}, khz[NCH] = {0, 0, 0};
                        src[at] = s, khz[at] = k;
                        const bool ok = mok && nsrc >= 0 && nsrc <= NCH && (nsrc == 0 || (s >= 0 && s < nsrc && k > -half && k <= half));
                        expect(sdr_tuner_check(mode, NCH, nsrc, src, khz), ok, "tuner", mode);
                    }
        const int32_t z[NCH] = {0, 0, 0};
        expect(sdr_tuner_check(mode, NCH, 1, nullptr, z), false, "tuner NULL src", mode);
        expect(sdr_tuner_check(mode, NCH, 1, z, nullptr), false, "tuner NULL khz", mode);
        expect(sdr_tuner_check(mode, NCH, 0, nullptr, nullptr), mok, "tuner untuned", mode);
    }
    for (int W : {4, 8, 10}) {
        // the smallest shift in 1..32 at which the peak rounds to at most the target, else 33; W's default for a peak of 0
        for (long long peak : {0LL, 1LL, 1LL << 31, (1LL << 33) - 1})
            for (int target : {1, 90, 127}) {
                int want = peak == 0 ? (W == 4 ? 22 : W == 8 ? 23 : 24) : 33;
                for (int s = 32; s >= 1 && peak > 0; s--)
                    if (((peak + (1LL << (s - 1))) >> s) <= target) want = s;
                const int s = sdr_split16_shift_for(peak, target, W);
                accepted++;
                if (s != want) {
                    std::printf("WRONG split16_shift_for(%lld, %d, %d) = %d, not %d\n", peak, target, W, s, want);
                    wrong++;
                }
            }
        expect(sdr_split16_shift_for(1, 90, W + 1), false, "split16_shift_for W", 0);
        expect(sdr_split16_shift_for(1, 0, W), false, "split16_shift_for target 0", 0);
        expect(sdr_split16_shift_for(1, 128, W), false, "split16_shift_for target 128", 0);
        expect(sdr_split16_shift_for(-1, 90, W), false, "split16_shift_for negative peak", 0);
        // the table: the count first, then the pairs into a vector of exactly that size (a builder that writes
        // past R T pairs is the sanitizer's to find), one pair too few refused, 14-bit entries
        int n = 0;
        expect(sdr_split_taps(W, nullptr, 0, &n), true, "split_taps count", 0);
        expect(sdr_split_taps(W, nullptr, 0, nullptr), false, "split_taps NULL n", 0);
        std::vector<int16_t> g((size_t)2 * n);
        expect(sdr_split_taps(W, g.data(), n - 1, &n), false, "split_taps short", 0);
        expect(sdr_split_taps(W, g.data(), n, &n), true, "split_taps", 0);
        int big = 0;
        for (int16_t e : g) big = std::abs((int)e) > big ? std::abs((int)e) : big;
        if (n != (2 * W - 1) * 16 * W || big == 0 || big > 8191) {
            std::printf("WRONG split_taps(%d): %d pairs, largest entry %d\n", W, n, big);
            wrong++;
        }
        // the tap fragments and the column sums: both creates build them from the table in front of their first
        // HIP call, which refuses device -1
        sdr_split* s8 = nullptr;
        sdr_split16* s16 = nullptr;
        const int rc8 = sdr_split_create(&s8, -1, 0, W, 2, 0), rc16 = sdr_split16_create(&s16, -1, 0, W, 2, 0);
        if (rc8 != SDR_E_HIP || rc16 != SDR_E_HIP || s8 || s16) {
            std::printf("WRONG creates on device -1 (W %d): rc %d and %d\n", W, rc8, rc16);
            wrong++;
        }
    }
    std::printf("opts_check_driver: %d accepted, %d refused, %d wrong\n", accepted, refused, wrong);
    return wrong ? 1 : 0;
}
