// validate_lf.cpp -- the lane-pair loop filter of sdr_pll.hip pll_step_split, evaluated here operation
// for operation on the host, against the reference's five operations (src/pll.cpp:41-42):
//   reference:  integ' = integ + RN(Ki e);  ph' = (ph + RN(Kp e)) + integ'
//   pair:       lane A (even, owns phaseEst):   s1A = ph + RN(Kp e)
//               lane B (odd, owns integrator):  s1B = integ + RN(Ki e)
//               both lanes: p = s1_own + s1_partner  (A: s1A + s1B, B: s1B + s1A);  A keeps p, B keeps s1B
// (one multiply, one add, one add with the partner's value, one select per lane: no fused operation).
// Both lanes' p, lane A's kept word and lane B's kept word must carry the reference's bits (any NaN
// equals any NaN: the payload is not part of the PLL's state checks, which reject every NaN).
// Inputs: N random (integ, ph, e) triples over the state ranges and beyond, every triple of a grid of
// specials (+-0, smallest and largest denormals, +-FLT_MIN, +-pi, +-inf, NaN, ...), constructed cases
// where ph + RN(Kp e) and s1A + s1B land exactly on a rounding tie, and chained runs where each lane
// carries its own word from step to step.
//   g++ -O2 -std=c++17 -ffp-contract=off tools/pllmath/validate_lf.cpp -o /tmp/validate_lf
//   /tmp/validate_lf [N]
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}
static bool same(float a, float b) { return (std::isnan(a) && std::isnan(b)) || bits(a) == bits(b); }

struct State {
    float integ, ph;
};

// src/pll.cpp:41-42
static State ref_step(State s, float e, float Kp, float Ki) {
    const float ki_e = Ki * e;
    const float integ = s.integ + ki_e;
    const float ph = (s.ph + Kp * e) + integ;
    return {integ, ph};
}

// the two lanes of a pair: each holds one word and one gain
struct Pair {
    float sA, sB;   // A: phaseEst, B: integrator
    float pA, pB;   // phaseEst' as each lane sees it (the value converted for trigArg)
};
static Pair pair_step(float sA, float sB, float e, float Kp, float Ki) {
    const float dA = Kp * e, dB = Ki * e;       // d = K * e
    const float s1A = sA + dA, s1B = sB + dB;   // s1 = s + d
    const float pA = s1A + s1B, pB = s1B + s1A; // p = s1 + pair_swap(s1)
    return {pA, s1B, pA, pB};                   // s = a ? p : s1
}

static long check(State s, float e, float Kp, float Ki) {
    const State r = ref_step(s, e, Kp, Ki);
    const Pair p = pair_step(s.ph, s.integ, e, Kp, Ki);
    return (same(p.sA, r.ph) && same(p.sB, r.integ) && same(p.pA, r.ph) && same(p.pB, r.ph)) ? 0 : 1;
}

int main(int argc, char** argv) {
    const long N = argc > 1 ? std::atol(argv[1]) : 10000000;
    std::mt19937_64 rng(4142);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    // the gains of the two PLLs as the kernels form them (normBandwidth * 2.666f, nb^2 * 3.555f)
    const float bws[] = {0.01f, 0.001f, 0.05f, 1.0f};
    auto Kp_of = [](float bw) { const float Cp = 2.666; return bw * Cp; };
    auto Ki_of = [](float bw) { const float Ci = 3.555; return bw * bw * Ci; };

    // 1. random triples: log-uniform magnitudes past both state ranges, e in [-pi, pi] and tiny
    long rnd_bad = 0;
    for (long i = 0; i < N; i++) {
        const float bw = bws[i & 3];
        auto mag = [&](double lo, double hi) { return (float)((U(rng) < 0.5 ? -1.0 : 1.0) * std::exp2(lo + (hi - lo) * U(rng))); };
        const float integ = mag(-150.0, 22.0), ph = mag(-150.0, 30.0);
        const float e = (i & 4) ? (float)((2.0 * U(rng) - 1.0) * 3.14159265358979) : mag(-150.0, 1.7);
        rnd_bad += check({integ, ph}, e, Kp_of(bw), Ki_of(bw));
    }

    // 2. the grid of specials, every triple, every bandwidth
    const float dmin = std::numeric_limits<float>::denorm_min();
    const float dmax = std::nextafterf(FLT_MIN, 0.0f);
    const float pi_f = 3.14159274f;
    std::vector<float> sp;
    for (float v : {0.0f, dmin, dmax, FLT_MIN, 2.0f * FLT_MIN, 0x1p-100f, 0x1p-24f, 1.0f, pi_f, std::nextafterf(pi_f, 0.0f),
                    0x1p20f, 0x1p24f, 0x1p28f, FLT_MAX, INFINITY}) {
        sp.push_back(v);
        sp.push_back(-v);
    }
    sp.push_back(NAN);
    long spec_n = 0, spec_bad = 0, negzero_n = 0;
    for (float bw : bws)
        for (float integ : sp)
            for (float ph : sp)
                for (float e : sp) {
                    spec_n++;
                    negzero_n += bits(integ) == 0x80000000u ? 1 : 0;   // the -0 integrator: no exception
                    spec_bad += check({integ, ph}, e, Kp_of(bw), Ki_of(bw));
                }

    // 3. rounding ties. e with RN(Kp e) = 2^k exactly and ph = +-(2^(k+24) [+ 2^(k+1)]) (ulp 2^(k+1),
    //    either parity of the last bit): ph + RN(Kp e) is a tie. With integ = +-2^k - RN(Ki e) (exact
    //    here: counted only when it is) the second sum s1A + s1B is a tie too. Ties are confirmed in
    //    double arithmetic (exact for these magnitudes) before they are counted.
    auto is_tie = [](float a, float b) { const double x = (double)a + (double)b; return (double)(float)x != x; };
    long tie_n = 0, tie2_n = 0, tie_bad = 0;
    for (float bw : bws) {
        const float Kp = Kp_of(bw), Ki = Ki_of(bw);
        for (int k = -20; k <= 1; k++) {
            const float want = std::ldexp(1.0f, k);
            float e = 0.0f;
            for (int j = -8; j <= 8; j++) {           // a neighbour of 2^k / Kp whose product rounds to 2^k
                float c = want / Kp;
                for (int t = 0; t < std::abs(j); t++) c = std::nextafterf(c, j < 0 ? 0.0f : INFINITY);
                if (Kp * c == want) e = c;
            }
            if (Kp * e != want || !(e < 3.1415925f)) continue;
            for (float sgn : {1.0f, -1.0f})
                for (int odd = 0; odd < 2; odd++)
                    for (float isg : {1.0f, -1.0f}) {
                        const float es = sgn * e;
                        const float ph = sgn * (std::ldexp(1.0f, k + 24) + (odd ? std::ldexp(1.0f, k + 1) : 0.0f));
                        const float integ = isg * want - Ki * es;
                        if (!is_tie(ph, Kp * es)) continue;
                        tie_n++;
                        tie_bad += check({0.0f, ph}, es, Kp, Ki);
                        tie_bad += check({integ, ph}, es, Kp, Ki);
                        if (is_tie(ph + Kp * es, integ + Ki * es)) tie2_n++;
                        // first sum exact, second a tie
                        const float ph2 = ph - Kp * es;
                        if (!is_tie(ph2, Kp * es) && is_tie(ph2 + Kp * es, integ + Ki * es)) tie2_n++;
                        tie_bad += check({integ, ph2}, es, Kp, Ki);
                    }
        }
    }

    // 4. chained: each lane carries its own word; 64 chains of 20000 steps per bandwidth
    long chain_n = 0, chain_bad = 0;
    for (float bw : bws) {
        const float Kp = Kp_of(bw), Ki = Ki_of(bw);
        for (int c = 0; c < 64; c++) {
            State r{c & 1 ? -0.0f : 0.0f, (float)(U(rng) - 0.5)};
            float sA = r.ph, sB = r.integ;
            const double drift = (U(rng) - 0.5) * 0.2;
            for (int i = 0; i < 20000; i++) {
                const float e = (c & 2) && i < 100 ? (i & 1 ? -0.0f : 0.0f) : (float)(drift + (U(rng) - 0.5) * 0.5);
                r = ref_step(r, e, Kp, Ki);
                const Pair p = pair_step(sA, sB, e, Kp, Ki);
                sA = p.sA;
                sB = p.sB;
                chain_n++;
                chain_bad += (same(sA, r.ph) && same(sB, r.integ) && same(p.pB, r.ph)) ? 0 : 1;
            }
        }
    }
    std::printf("{\"n\": %ld, \"mismatch\": %ld, \"specials\": %ld, \"special_mismatch\": %ld, \"negzero_integ\": %ld, "
                "\"ties\": %ld, \"ties_second_sum\": %ld, \"tie_mismatch\": %ld, \"chain_steps\": %ld, \"chain_mismatch\": %ld}\n",
                N, rnd_bad, spec_n, spec_bad, negzero_n, tie_n, tie2_n, tie_bad, chain_n, chain_bad);
    return (rnd_bad | spec_bad | tie_bad | chain_bad) == 0 ? 0 : 1;
}
