// pll_chunk_proof_driver.cpp -- which 16-step chunks of a PLL input the fast lane-pair step cannot
// prove (sdr_pll.hip pair_chunk redoes exactly those with the checked step), decided on the host
// with pll_math.h, for tests/test_gpu_pll_chunk.py.
//
// The reference recurrence (pll.cpp:34-50, glibc atan2 / cos / sin) carries the state; before each
// of its steps the fast step's proof obligations are evaluated on that state, operation for
// operation as sdr_pll.hip pll_step_split does (tools/pllmath/validate_e3.cpp states the same
// phase detector): the previous trigArg in the reduction's range with both roundings of cos r,
// sin r clear of an f32 tie (tie_key64 > TIE_MIN), the e bracket RN32(ed - eps) == RN32(ed) ==
// RN32(ed + eps), |RN32(ed)| below the e range, and at the chunk's end |phaseEst| < 2^28 and
// |integrator| < 2^20. A chunk with one failed obligation is one the kernel redoes; the obligations
// of a step hold for the kernel's state as long as every earlier one of the chunk held, so the first
// failure of a chunk is exact and that is all that is counted.
//   driver FREQ FS BW N < x.f32    ->  "chunks failed" on stdout
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pll_math.h"

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const float freq = (float)std::atof(argv[1]), Fs = (float)std::atof(argv[2]), bw = (float)std::atof(argv[3]);
    const int n = std::atoi(argv[4]);
    std::vector<float> x((size_t)n);
    if (std::fread(x.data(), sizeof(float), (size_t)n, stdin) != (size_t)n) return 3;
    const float Cp = 2.666;
    const float Ci = 3.555;
    const float Kp = bw * Cp;
    const float Ki = bw * bw * Ci;
    const double w = 2 * 3.14159265358979323846 * (freq / Fs);
    const uint32_t emax_bits = 0x40490FDAu;   // the largest f32 below pi - 2^-30 (sdr_pll.hip PLL_EMAX_F)
    float emax_f;
    std::memcpy(&emax_f, &emax_bits, sizeof emax_f);
    float fbI = 1.0f, fbQ = 0.0f, integ = 0.0f, ph = 0.0f;
    double toff = 0.0;
    const int C = 16;
    int chunks = 0, failed = 0;
    for (int i0 = 0; i0 + C <= n; i0 += C) {
        bool bad = false;
        for (int j = 0; j < C; j++) {
            const float xi = x[(size_t)(i0 + j)];
            const float t_prev = (float)(w * toff + (double)ph);
            const pllm::SinCosRN sc = pllm::sincos_rn(t_prev);
            if (!(std::fabs((double)t_prev) < pllm::T_MAX && sc.tie > pllm::TIE_MIN)) bad = true;
            const float gA = -xi * (float)sc.sr, gB = xi * (float)sc.cr;
            const double Y = (double)gA * sc.cr + (double)gB * sc.sr;
            const double rx = pllm::pll_rx(xi);
            const double ed = pllm::fma_(Y, rx, pllm::base_angle_n(pllm::lo_word(rx), sc.nq1, sc.b, -sc.r));
            const float e = (float)ed;
            if (!((float)(ed - pllm::EPS_ABS_E2) == e && (float)(ed + pllm::EPS_ABS_E2) == e && std::fabs(e) < emax_f))
                bad = true;
            // pll.cpp:36-50
            const float eI = xi * fbI, eQ = xi * (-fbQ);
            const float er = (float)std::atan2((double)eQ, (double)eI);
            integ = integ + Ki * er;
            ph = ph + Kp * er + integ;
            toff += 1.0;
            const float t = (float)(w * toff + (double)ph);
            fbI = (float)std::cos((double)t);
            fbQ = (float)std::sin((double)t);
        }
        if (!(std::fabs(ph) < 0x1p28f && std::fabs(integ) < 0x1p20f)) bad = true;
        chunks++;
        failed += bad ? 1 : 0;
    }
    std::printf("%d %d\n", chunks, failed);
    return 0;
}
