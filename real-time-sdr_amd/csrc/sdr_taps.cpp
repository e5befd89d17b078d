// sdr_taps.cpp -- host-side tap design of libsdr_amd.so (runs once per context, on the CPU).
//
// The filters are part of the reference's per-thread setup, not of the per-block hot path; the
// kernels only consume the taps. Each formula keeps the reference's operand types so the taps are
// bit-identical (compiled with -ffp-contract=off, no fast-math):
//   impulseResponseLPF  src/filter.cpp:13-29 (4-arg) and :33-50 (5-arg, integer gain u)
//   impulseResponseBPF  src/filter.cpp:55-71 (integer (num_taps-1)/2 in the sinc argument, :66)
//   impulseResponseAPF  src/filter.cpp:73-78
//   impulseResponseRRC  src/filter.cpp:80-102
#include <cmath>
#include <cstddef>

#include "sdr_amd.h"

#pragma clang fp contract(off)

namespace {
constexpr double kPi = 3.14159265358979323846;  // include/dy4.h:13
}

extern "C" int sdr_impulse_response_lpf(float Fs, float Fc, unsigned short num_taps, float* h) {
    if (!h || num_taps == 0) return SDR_E_INVALID;
    const float cutoff = Fc / (Fs / 2.0);
    const double centre = (num_taps - 1.0) / 2.0;
    for (int i = 0; i < num_taps; i++) {
        float v;
        if (i == centre) {
            v = cutoff;
        } else {
            const double arg = kPi * cutoff * (i - centre);
            v = cutoff * std::sin(arg) / (kPi * cutoff * (i - centre));
        }
        const double w = std::sin(i * kPi / ((float)num_taps));
        v = v * w * w;
        h[i] = v;
    }
    return SDR_OK;
}

extern "C" int sdr_impulse_response_lpf_gain(float Fs, float Fc, unsigned short num_taps, int u, float* h) {
    if (!h || num_taps == 0) return SDR_E_INVALID;
    const float cutoff = Fc / (Fs / 2.0);
    const double centre = (num_taps - 1.0) / 2.0;
    for (int i = 0; i < num_taps; i++) {
        float v;
        const float gain_cut = u * cutoff;  // the reference multiplies u*cutoff in float first
        if (i == centre) {
            v = gain_cut;
        } else {
            v = gain_cut * std::sin(kPi * cutoff * (i - centre)) / (kPi * cutoff * (i - centre));
        }
        const double w = std::sin(i * kPi / ((float)num_taps));
        v = v * w * w;
        h[i] = v;
    }
    return SDR_OK;
}

extern "C" int sdr_impulse_response_bpf(float Fs, const float* Fb, unsigned short num_taps, float* h) {
    if (!h || !Fb || num_taps == 0) return SDR_E_INVALID;
    const float centre_norm = ((Fb[1] + Fb[0]) / 2) / (Fs / 2);
    const float pass_norm = ((Fb[1] - Fb[0])) / (Fs / 2);
    for (int i = 0; i < num_taps; i++) {
        float v;
        if (i == (num_taps - 1.0) / 2.0) {
            v = pass_norm;
        } else {
            const int m = i - (num_taps - 1) / 2;
            v = pass_norm * ((std::sin(kPi * (pass_norm / 2) * m)) / (kPi * (pass_norm / 2) * m));
        }
        v = v * std::cos(i * kPi * centre_norm);
        const double w = std::sin(i * kPi / ((float)num_taps));
        v = v * w * w;
        h[i] = v;
    }
    return SDR_OK;
}

extern "C" int sdr_impulse_response_apf(float gain, unsigned short num_taps, float* h) {
    if (!h || num_taps == 0) return SDR_E_INVALID;
    for (int i = 0; i < num_taps; i++) h[i] = 0.0f;
    h[(std::size_t)((num_taps - 1.0) / 2.0)] = gain;
    return SDR_OK;
}

extern "C" int sdr_impulse_response_rrc(float Fs, unsigned short num_taps, float* h) {
    if (!h || num_taps == 0) return SDR_E_INVALID;
    const float T_symbol = 1 / 2375.0;
    const float beta = 0.90;
    for (int i = 0; i < num_taps; i++) {
        const float t = (i - (float)num_taps / 2.0) / Fs;
        if (t == 0.0) {
            h[i] = 1.0 + beta * ((4.0 / kPi) - 1);
        } else if ((t == (-T_symbol / (4.0 * beta))) | (t == (T_symbol / (4.0 * beta)))) {
            h[i] = (beta / std::sqrt(2.0)) * ((1 - 2.0 / kPi) * (std::sin(kPi / (4.0 * beta)))) +
                   ((1 - 2.0 / kPi) * (std::cos(kPi / (4 * beta))));
        } else {
            const double a = 4.0 * beta * t / T_symbol;
            h[i] = (std::sin(kPi * t * (1 - beta) / T_symbol) +
                    4.0 * beta * (t / T_symbol) * std::cos(kPi * t * (1 + beta) / T_symbol)) /
                   (kPi * t * (1 - a * a) / T_symbol);
        }
    }
    return SDR_OK;
}

// The shared-capture tuner's rotator table of a mode: T[i] = (cos, sin)(2 pi i / N), N = rf_Fs / 1000,
// each the real value correctly rounded to f32. Only the first octant is evaluated (in extended
// precision: the value's distance from an f32 rounding tie is then many orders above the evaluation
// error; tests/test_tuner_model.py compares every entry with a 50-digit evaluation); the rest follows
// by symmetry, so T[0] = (1, 0) and T[N/4] = (0, 1) exactly. A negated zero is written as 0 - x = +0.
// The kernel keeps the first half (the second is the first negated).
namespace {
int tuner_n(int mode) { return mode == 0 || mode == 2 ? 2400 : mode == 1 ? 1440 : mode == 3 ? 1152 : 0; }
}  // namespace

// Q[k] = RN32(cos(2 pi k / n)), 0 <= k <= n/4; sin(2 pi k / n) = Q[n/4 - k]
static int tuner_quarter(int n, float* q) {
    if (n <= 0 || n % 8 || !q) return SDR_E_INVALID;
    const long double two_pi = 6.283185307179586476925286766559005768L;
    const int q4 = n / 4, q8 = n / 8;
    for (int k = 0; k <= q8; k++) {
        const long double a = two_pi * (long double)k / (long double)n;
        q[k] = k == 0 ? 1.0f : (float)cosl(a);
        q[q4 - k] = k == 0 ? 0.0f : (float)sinl(a);   // cos(pi/2 - a); k = n/8 writes cos last
    }
    q[q8] = (float)cosl(two_pi * (long double)q8 / (long double)n);
    return SDR_OK;
}

extern "C" int sdr_tuner_table(int mode, float* cs, int max_pairs, int* n) {
    const int N = tuner_n(mode);
    if (N == 0 || !n) return SDR_E_INVALID;
    if (cs && max_pairs < N) return SDR_E_INVALID;
    *n = N;
    if (!cs) return SDR_OK;
    const int q4 = N / 4;
    float* q = new float[q4 + 1];
    tuner_quarter(N, q);
    for (int i = 0; i < N; i++) {
        const int qd = i / q4, r = i - qd * q4;
        const float a = q[r], b = q[q4 - r];            // cos and sin of 2 pi r / N
        float c = (qd & 1) ? b : a, s = (qd & 1) ? a : b;
        if (qd == 1 || qd == 2) c = 0.0f - c;
        if (qd >= 2) s = 0.0f - s;
        cs[2 * i] = c;
        cs[2 * i + 1] = s;
    }
    delete[] q;
    return SDR_OK;
}
