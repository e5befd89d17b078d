// Stand-alone driver of the RDS text layer (real-time-sdr_amd/csrc/sdr_rds_text.cpp) for a sanitizer run:
// random group records with random ok masks through sdr_rds_station_update and sdr_rds_station_format,
// into buffers of every small size. Compiled together with the text layer's source; no GPU, no library.
//   rds_station_driver [records] [seed]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "sdr_amd.h"

int main(int argc, char** argv) {
    const long n = argc > 1 ? std::atol(argv[1]) : 1000000;
    const unsigned seed = argc > 2 ? (unsigned)std::atol(argv[2]) : 1u;
    std::mt19937_64 rng(seed);
    sdr_rds_station st;
    sdr_rds_station_init(&st);
    unsigned long long sum = 0;
    size_t longest = 0;
    for (long k = 0; k < n; k++) {
        const uint64_t a = rng(), b = rng();
        sdr_rds_group g;
        std::memcpy(&g, &a, 8);
        std::memcpy((char*)&g + 8, &b, 8);
        // a third of the records are well-formed type 0, 2 and 4 groups, so the fields fill up
        if (k % 3 == 0) {
            static const uint16_t types[3] = {0x0000, 0x2000, 0x4000};
            g.w[1] = (uint16_t)((g.w[1] & 0x0FFF) | types[(k / 3) % 3]);
            g.flags &= 1;
        }
        sdr_rds_station_update(&st, &g);
        if ((k & 63) == 0 || k == n - 1) {
            // exact-size heap buffers: a write past the end is the sanitizer's to see
            const size_t cap = (size_t)(rng() % 700);
            std::vector<char> buf(cap ? cap : 1, 'x');
            const size_t need = sdr_rds_station_format(&st, cap ? buf.data() : nullptr, cap);
            if (need > longest) longest = need;
            if (cap) {
                if (std::strlen(buf.data()) >= cap) return 2;
                for (const char* p = buf.data(); *p; p++) sum += (unsigned char)*p;
            }
        }
        if ((k & 0xFFFF) == 0xFFFF) {
            sdr_rds_stats s;
            std::memcpy(&s, &a, 8);
            std::memset((char*)&s + 8, 0xFF, sizeof s - 8);
            sdr_rds_station_stats(&st, &s);
            if (!(sdr_rds_station_bler(&st) >= 0.0 && sdr_rds_station_bler(&st) <= 1.0)) return 3;
        }
    }
    sdr_rds_station_update(nullptr, nullptr);
    sdr_rds_station_update(&st, nullptr);
    sdr_rds_station_format(nullptr, nullptr, 0);
    std::printf("sizeof %zu records %ld groups %u longest %zu sum %llu\n", sizeof(sdr_rds_station), n, st.ngroups, longest,
                sum);
    return 0;
}
