// validate_step2.cpp -- the whole lane-pair PLL step of sdr_pll.hip (pll_step_split) and its chunk
// verdict (pair_chunk), evaluated here operation for operation on the host, both lanes modelled,
// against the reference step (src/pll.cpp:36-50) evaluated with glibc's f64 atan2 / cos / sin.
//
// A chunk is 16 steps from one state. The model runs them as the kernel does -- the phase detector
// across the pair (g = RN32(xs fb_partner), q = g f_own, Y = q + q_partner, ed = fma(Y, rx, base)),
// one loop-filter word per lane, t = RN32(w toff + ph), the two-fma reduction, each lane's kernel
// f = u + z u P(z) by Horner -- and accumulates the kernel's proofs: each lane's end of the e bracket,
// each lane's tie key, the largest |t|, and at the chunk's end the range of each lane's state word.
// An accepted chunk (every proof of both lanes holds, the kernel's `pair_ok`) must give the
// reference's 16 phases t and its end state bit for bit; a rejected chunk is the checked step's
// business (tests/test_gpu_pll_chunk.py) and is only counted. The |e| < pi - 2^-30 test that the
// chunk carried until round 14 is evaluated beside the proofs, not among them: "e_range_only" counts
// the accepted chunks it would have rejected, and they are compared like every other accepted chunk
// (pll_math.h, "The cut at +-pi").
//
// Chunks: random states (trigOffset up to 1.5e8 samples at both PLL configurations, so |t| runs up
// to 2^28.7; phaseEst, integrator of either sign) with 16 inputs of one kind each: a tone the loop
// tracks, inputs of random sign and magnitude down to 2^-40 (e anywhere in [-pi, pi]), and inputs
// with zeros, -0, denormals, values below pll_rx's 2^-60, FLT_MAX, inf and NaN mixed in.
// Special chunks: the previous trigArg on and within 3 ulps of the f32 neighbours of k pi/2,
// |k| <= 8 (|r| ~ 2^-24: base is within 2^-22 of +-pi for the matching quadrant and input sign, the
// e range's edge), with inputs of both signs, of ordinary size and down at 2^-60 (x fQ0 underflows: the
// sign of a subnormal or zero eQ decides the reference's side of the cut); and states whose words sit
// next to their range bounds.
//
// STEP2_POLY (0: the shipped Horner; 1: Estrin; 2: Horner in z^2 of three linear pieces) and
// STEP2_OWN (1: ed = fma(q_partner, rx, fma(q_own, rx, base)) with both bracket ends per lane)
// evaluate the orders that profiles/r15/pll_step2/ measured and did not keep.
//   g++ -O2 -std=c++17 -ffp-contract=off -I real-time-sdr_amd/csrc tools/pllmath/validate_step2.cpp -o /tmp/validate_step2
//   /tmp/validate_step2 [N steps]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "pll_math.h"

#ifndef STEP2_POLY
#define STEP2_POLY 0
#endif
#ifndef STEP2_OWN
#define STEP2_OWN 0
#endif

namespace {
constexpr int C = 16;                                                  // PLL_CHUNK
constexpr float PLL_EMAX_F = 3.14159250259399414062f;                  // 0x40490FDA (sdr_pll.hip)
constexpr double FS = 240000.0;

uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }
bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }

struct RefState { float fbI, fbQ, integ, ph; double toff; };

// src/pll.cpp:36-50, one step; returns trigArg
float ref_step(RefState& s, float x, float Kp, float Ki, double w) {
    const float eI = x * s.fbI;
    const float eQ = x * (-s.fbQ);
    const float e = (float)std::atan2((double)eQ, (double)eI);
    s.integ = s.integ + Ki * e;
    s.ph = s.ph + Kp * e + s.integ;
    s.toff += 1.0;
    const float t = (float)(w * s.toff + (double)s.ph);
    s.fbI = (float)std::cos((double)t);
    s.fbQ = (float)std::sin((double)t);
    return t;
}

struct LaneConst { double c[6], k1, k0, eps; float K, smax; };
struct Lane { double f; float fb, s; uint32_t split, tie; };
struct Pair {                                                          // SplitRegs of both lanes
    Lane A, B;
    double toff, mr;
    uint32_t nq1, b;
};

LaneConst lane_const(bool a, float Kp, float Ki) {                      // split_lane
    LaneConst L;
    if (a) L = {{-0.5, pllm::C1, pllm::C2, pllm::C3, pllm::C4, pllm::C5}, 0.0, 1.0, -pllm::EPS_ABS_E2, Kp, 0x1p28f};
    else   L = {{pllm::S1, pllm::S2, pllm::S3, pllm::S4, pllm::S5, pllm::S6}, 1.0, 0.0, pllm::EPS_ABS_E2, Ki, 0x1p20f};
    return L;
}

double poly(const LaneConst& L, double z) {
#if STEP2_POLY == 2
    const double z2 = z * z;
    const double p01 = pllm::fma_(z, L.c[1], L.c[0]), p23 = pllm::fma_(z, L.c[3], L.c[2]), p45 = pllm::fma_(z, L.c[5], L.c[4]);
    return pllm::fma_(z2, pllm::fma_(z2, p45, p23), p01);
#elif STEP2_POLY == 1
    const double z2 = z * z, z4 = z2 * z2;
    const double p01 = pllm::fma_(z, L.c[1], L.c[0]), p23 = pllm::fma_(z, L.c[3], L.c[2]), p45 = pllm::fma_(z, L.c[5], L.c[4]);
    return pllm::fma_(z4, p45, pllm::fma_(z2, p23, p01));
#else
    double P = pllm::fma_(z, L.c[5], L.c[4]);
    P = pllm::fma_(z, P, L.c[3]);
    P = pllm::fma_(z, P, L.c[2]);
    P = pllm::fma_(z, P, L.c[1]);
    return pllm::fma_(z, P, L.c[0]);
#endif
}

struct Proof { float emaxf = 0.0f, tmax = 0.0f; bool lanes_agree = true; };

// pll_step_split on both lanes; xs = -x on lane A, x on lane B
float pair_step(Pair& p, float x, double rx, double w, Proof& pf, const LaneConst& LA, const LaneConst& LB) {
    const float gA = (-x) * p.B.fb, gB = x * p.A.fb;
    const double qA = (double)gA * p.A.f, qB = (double)gB * p.B.f;
    const double base = pllm::base_angle_n(pllm::lo_word(rx), p.nq1, p.b, p.mr);
#if STEP2_OWN
    const double edA = pllm::fma_(qB, rx, pllm::fma_(qA, rx, base)), edB = pllm::fma_(qA, rx, pllm::fma_(qB, rx, base));
#else
    const double edA = pllm::fma_(qA + qB, rx, base), edB = pllm::fma_(qB + qA, rx, base);
#endif
    const float eA = (float)edA, eB = (float)edB;
    if (!same(eA, eB)) pf.lanes_agree = false;                          // the kernel never compares them
    pf.emaxf = std::fmax(pf.emaxf, std::fabs(eA));
    pf.emaxf = std::fmax(pf.emaxf, std::fabs(eB));
    const float s1A = p.A.s + LA.K * eA, s1B = p.B.s + LB.K * eB;
    p.A.split |= bits((float)(edA + LA.eps)) ^ bits(eA);
    p.B.split |= bits((float)(edB + LB.eps)) ^ bits(eB);
#if STEP2_OWN
    p.A.split |= bits((float)(edA - LA.eps)) ^ bits(eA);
    p.B.split |= bits((float)(edB - LB.eps)) ^ bits(eB);
#endif
    const float ph = s1A + s1B;                                         // the same bits on both lanes: f32 add commutes
    p.A.s = ph;
    p.B.s = s1B;
    p.toff += 1.0;
    const float t = (float)(w * p.toff + (double)ph);
    const double xt = (double)t;
    const double kdp = pllm::fma_(xt, -pllm::TWO_OVER_PI, pllm::MAGIC1);
    const double kdn = kdp - pllm::MAGIC1;
    const double rr = pllm::fma_(kdn, pllm::PIO2_LO, pllm::fma_(kdn, pllm::PIO2_HI, xt));
    p.nq1 = (uint32_t)__builtin_bit_cast(uint64_t, kdp);
    p.b = (uint32_t)(__builtin_bit_cast(uint64_t, rr) >> 63);
    p.mr = -rr;
    const double z = rr * rr;
    for (int l = 0; l < 2; l++) {
        const LaneConst& L = l ? LB : LA;
        Lane& ln = l ? p.B : p.A;
        const double u = pllm::fma_(rr, L.k1, L.k0);
        ln.f = pllm::fma_(z * u, poly(L, z), u);
        ln.fb = (float)ln.f;
        const uint32_t key = pllm::tie_key64(ln.f);
        ln.tie = key < ln.tie ? key : ln.tie;
    }
    pf.tmax = std::fmax(pf.tmax, std::fabs(t));
    return t;
}

// pll_load: the pair's registers from a state whose feedback is RN32(cos t), RN32(sin t) of its own t
bool pair_load(Pair& p, const RefState& s, double w) {
    const float t_prev = (float)(w * s.toff + (double)s.ph);
    const pllm::SinCosRN sc = pllm::sincos_rn(t_prev);
    float fI = (float)sc.cr, fQ = (float)sc.sr;
    pllm::rot_q(1u - sc.nq1, fI, fQ);
    if (!((std::fabs((double)t_prev) < pllm::T_MAX) && sc.tie > pllm::TIE_MIN && fI == s.fbI && fQ == s.fbQ)) return false;
    p.A = {sc.cr, (float)sc.cr, s.ph, 0u, ~0u};
    p.B = {sc.sr, (float)sc.sr, s.integ, 0u, ~0u};
    p.toff = s.toff;
    p.mr = -sc.r;
    p.nq1 = sc.nq1;
    p.b = sc.b;
    return true;
}

struct Totals {
    long chunks = 0, accepted = 0, steps_accepted = 0, wrong_steps = 0, wrong_state = 0, lanes_disagree = 0;
    long rej_emax = 0, rej_split = 0, rej_tie = 0, rej_state = 0, rej_t = 0, unloadable = 0;
    long emax_only = 0;       // accepted chunks that the former e range test would have rejected
    long emax_only_wrong = 0; // ... of which the fast results differ from the reference's (counted in wrong_* too)
};

void run_chunk(RefState s, const float* x, float bw, float freq, Totals& T) {
    const float Kp = bw * 2.666f, Ki = bw * bw * 3.555f;
    const double w = 2 * 3.14159265358979323846 * (freq / (float)FS);
    Pair p;
    if (!pair_load(p, s, w)) { T.unloadable++; return; }
    const LaneConst LA = lane_const(true, Kp, Ki), LB = lane_const(false, Kp, Ki);
    Proof pf;
    float tf[C], tr[C];
    for (int j = 0; j < C; j++) {
        tf[j] = pair_step(p, x[j], pllm::pll_rx(x[j]), w, pf, LA, LB);
        tr[j] = ref_step(s, x[j], Kp, Ki, w);
    }
    const bool emax_ok = pf.emaxf < PLL_EMAX_F;
    const bool split_ok = p.A.split == 0u && p.B.split == 0u;
    const bool tie_ok = p.A.tie > pllm::TIE_MIN && p.B.tie > pllm::TIE_MIN;
    const bool state_ok = std::fabs(p.A.s) < LA.smax && std::fabs(p.B.s) < LB.smax;
    const bool t_ok = pf.tmax < 0x1p30f;
    T.chunks++;
    T.rej_emax += !emax_ok; T.rej_split += !split_ok; T.rej_tie += !tie_ok; T.rej_state += !state_ok; T.rej_t += !t_ok;
    long wrong = 0;
    for (int j = 0; j < C; j++) wrong += !same(tf[j], tr[j]);
    float fI = p.A.fb, fQ = p.B.fb;
    pllm::rot_q(1u - p.nq1, fI, fQ);
    const bool state_same = same(fI, s.fbI) && same(fQ, s.fbQ) && same(p.A.s, s.ph) && same(p.B.s, s.integ) && p.toff == s.toff;
    if (!(split_ok && tie_ok && state_ok && t_ok)) return;
    if (!emax_ok) {
        T.emax_only++;
        T.emax_only_wrong += (wrong != 0 || !state_same);
    }
    T.accepted++;
    T.steps_accepted += C;
    T.wrong_steps += wrong;
    T.wrong_state += !state_same;
    T.lanes_disagree += !pf.lanes_agree;
}
}  // namespace

int main(int argc, char** argv) {
    const long N = argc > 1 ? std::atol(argv[1]) : 20000000;
    std::mt19937_64 rng(1502);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const float cfg[2][2] = {{19e3f, 0.01f}, {114e3f, 0.001f}};        // stereo.cpp:77, rds.cpp:119
    const float inf = std::numeric_limits<float>::infinity();
    const float odd[] = {0.0f, -0.0f, 1e-45f, -1e-45f, 1.17549421e-38f, 0x1p-61f, -0x1p-61f, 0x1p-60f, -0x1p-60f,
                         3.4028234663852886e38f, -3.4028234663852886e38f, inf, -inf, std::nanf("")};
    Totals R, S;                                                       // random, special
    auto state_at = [&](float freq, double toff, float ph, float integ) {
        RefState s;
        s.toff = toff; s.ph = ph; s.integ = integ;
        const double w = 2 * 3.14159265358979323846 * (freq / (float)FS);
        const float t = (float)(w * toff + (double)ph);
        s.fbI = (float)std::cos((double)t);
        s.fbQ = (float)std::sin((double)t);
        return s;
    };
    // ---- random chunks
    while (R.chunks * C < N) {
        const int k = (int)(U(rng) * 2.0) & 1;
        const float freq = cfg[k][0], bw = cfg[k][1];
        const double toff = std::floor(std::exp2(28.0 * U(rng)) * 0.56);
        const float ph = (float)((U(rng) - 0.5) * std::exp2(-6.0 + 14.0 * U(rng)));
        const float integ = (float)((U(rng) - 0.5) * std::exp2(-12.0 + 10.0 * U(rng)));
        const RefState s = state_at(freq, toff, ph, integ);
        float x[C];
        const int kind = (int)(U(rng) * 8.0);
        const double amp = std::exp2(-8.0 * U(rng)), det = 6.0 * (U(rng) - 0.5), p0 = 6.283185307179586 * U(rng);
        const double w = 2 * 3.14159265358979323846 * (freq / (float)FS);
        for (int j = 0; j < C; j++) {
            if (kind < 4)          // a tone near the loop's own phase, with noise: small e, the locked case
                x[j] = (float)(amp * (std::cos(w * (toff + 1.0 + j) + (double)ph + 0.05 * det * j + (kind < 2 ? 0.0 : p0)) + 0.05 * (U(rng) - 0.5)));
            else if (kind < 7)     // any sign and magnitude: e anywhere in [-pi, pi]
                x[j] = (float)((U(rng) - 0.5) * std::exp2(-40.0 * U(rng) * U(rng)));
            else                   // odd values mixed in
                x[j] = U(rng) < 0.25 ? odd[(int)(U(rng) * (sizeof odd / sizeof *odd))] : (float)(U(rng) - 0.5);
        }
        run_chunk(s, x, bw, freq, R);
    }
    // ---- special chunks: trigArg next to k pi/2 (toff = 0: t_prev = phaseEst), inputs of both signs
    for (int k = -8; k <= 8; k++)
        for (int du = -3; du <= 3; du++)
            for (int c = 0; c < 2; c++)
                for (int rep = 0; rep < 64; rep++) {
                    float ph = (float)(k * pllm::PIO2);
                    for (int i = 0; i < std::abs(du); i++) ph = std::nextafterf(ph, du > 0 ? inf : -inf);
                    const RefState s = state_at(cfg[c][0], 0.0, ph, (float)((U(rng) - 0.5) * 1e-3));
                    float x[C];
                    // sign by rep; |x| in [0.01, 1], or down at pll_rx's 2^-60 where x fQ0 underflows
                    for (int j = 0; j < C; j++)
                        x[j] = (float)((rep & 1 ? -1.0 : 1.0) * (0.01 + U(rng)) * (rep & 2 && j ? (U(rng) - 0.5) : 1.0) *
                                       (rep & 4 ? 0x1p-53 : 1.0));
                    run_chunk(s, x, cfg[c][1], cfg[c][0], S);
                }
    // ---- special chunks: the state words next to their range bounds (2^28, 2^20)
    for (int c = 0; c < 2; c++)
        for (int sg = -1; sg <= 1; sg += 2)
            for (int rep = 0; rep < 256; rep++) {
                const float ph = sg * (rep & 1 ? std::nextafterf(0x1p28f, 0.0f) : 0x1p28f - 64.0f * (float)rep);
                const float integ = sg * (rep & 2 ? std::nextafterf(0x1p20f, 0.0f) : (float)(U(rng) * 1e-3));
                const RefState s = state_at(cfg[c][0], std::floor(U(rng) * 1e6), rep & 4 ? (float)(U(rng) - 0.5) : ph, integ);
                float x[C];
                for (int j = 0; j < C; j++) x[j] = (float)(U(rng) - 0.5);
                run_chunk(s, x, cfg[c][1], cfg[c][0], S);
            }
    const long wrong = R.wrong_steps + R.wrong_state + S.wrong_steps + S.wrong_state;
    std::printf("{\"poly\": %d, \"own\": %d, \"steps\": %ld, \"chunks\": %ld, \"accepted_chunks\": %ld, \"accepted_steps\": %ld, "
                "\"wrong_steps\": %ld, \"wrong_state\": %ld, \"lanes_disagree\": %ld, \"unloadable\": %ld, "
                "\"rejected\": {\"e_range\": %ld, \"e_bracket\": %ld, \"tie\": %ld, \"state\": %ld, \"t\": %ld}, "
                "\"special_chunks\": %ld, \"special_accepted\": %ld, \"special_wrong\": %ld, \"special_e_range\": %ld, "
                "\"e_range_only\": %ld, \"e_range_only_wrong\": %ld}\n",
                STEP2_POLY, STEP2_OWN, R.chunks * C, R.chunks, R.accepted, R.steps_accepted, R.wrong_steps, R.wrong_state,
                R.lanes_disagree + S.lanes_disagree, R.unloadable + S.unloadable, R.rej_emax, R.rej_split, R.rej_tie, R.rej_state,
                R.rej_t, S.chunks, S.accepted, S.wrong_steps + S.wrong_state, S.rej_emax, R.emax_only + S.emax_only,
                R.emax_only_wrong + S.emax_only_wrong);
    return wrong == 0 ? 0 : 1;
}
