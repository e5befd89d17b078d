// opts_check_driver.cpp -- every sdr_*_check function of libsdr_amd.so (include/sdr_amd.h) over the grid of
// tests/test_opts_check.py, and a NULL for each pointer argument: a stand-alone program for a sanitizer run of
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
#include <initializer_list>
#include <limits>

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
    std::printf("opts_check_driver: %d accepted, %d refused, %d wrong\n", accepted, refused, wrong);
    return wrong ? 1 : 0;
}
