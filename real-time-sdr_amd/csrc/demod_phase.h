// demod_phase.h -- the phase discriminator (SDR_FLAG_PHASE_DEMOD, include/sdr_amd.h; the numpy model
// tests/demod_model.py is the definition): atan2(im, re) of re + j im = x[n] conj(x[n-1]) in f32, every
// product, sum and quotient rounded on its own. The units that include it are compiled with
// -ffp-contract=off, so nothing here becomes an FMA except inside the expansion of the correctly
// rounded division (hipcc's default for f32 `/`, subnormals kept).
#pragma once

#include "sdr_internal.h"

namespace sdrk SDRK_HIDDEN {

// Two outputs at once: the quotient's operands are selected per output, the polynomial in u = z^2 runs
// on the packed pair (v_pk_mul_f32 / v_pk_add_f32, the coefficients as constants).
__device__ __forceinline__ f32x2 demod_phase2(f32x2 re, f32x2 im) {
    const f32x2 a = f32x2{__builtin_fabsf(re.x), __builtin_fabsf(re.y)};
    const f32x2 b = f32x2{__builtin_fabsf(im.x), __builtin_fabsf(im.y)};
    const bool sw0 = b.x > a.x, sw1 = b.y > a.y;
    const f32x2 mx = f32x2{sw0 ? b.x : a.x, sw1 ? b.y : a.y};
    const f32x2 mn = f32x2{sw0 ? a.x : b.x, sw1 ? a.y : b.y};
    const f32x2 z = f32x2{mn.x / mx.x, mn.y / mx.y};   // 0 / 0 = NaN where mx == 0: replaced below
    const f32x2 u = z * z;
    f32x2 p = f32x2{SDR_DEMOD_C7, SDR_DEMOD_C7};
    p = p * u + f32x2{SDR_DEMOD_C6, SDR_DEMOD_C6};
    p = p * u + f32x2{SDR_DEMOD_C5, SDR_DEMOD_C5};
    p = p * u + f32x2{SDR_DEMOD_C4, SDR_DEMOD_C4};
    p = p * u + f32x2{SDR_DEMOD_C3, SDR_DEMOD_C3};
    p = p * u + f32x2{SDR_DEMOD_C2, SDR_DEMOD_C2};
    p = p * u + f32x2{SDR_DEMOD_C1, SDR_DEMOD_C1};
    p = p * u + f32x2{SDR_DEMOD_C0, SDR_DEMOD_C0};
    f32x2 r = p * z;
    const f32x2 rh = f32x2{SDR_DEMOD_PI_2, SDR_DEMOD_PI_2} - r;
    r = f32x2{sw0 ? rh.x : r.x, sw1 ? rh.y : r.y};
    const f32x2 rp = f32x2{SDR_DEMOD_PI, SDR_DEMOD_PI} - r;
    r = f32x2{re.x < 0.0f ? rp.x : r.x, re.y < 0.0f ? rp.y : r.y};
    return f32x2{mx.x == 0.0f ? 0.0f : __builtin_copysignf(r.x, im.x),
                 mx.y == 0.0f ? 0.0f : __builtin_copysignf(r.y, im.y)};
}

// (re, im) of x conj(x_prev): cur = (I, Q), pv = (Ip, Qp)
__device__ __forceinline__ void demod_products(f32x2 cur, f32x2 pv, float& re, float& im) {
    const f32x2 d = cur * pv;                          // (I Ip, Q Qp)
    const f32x2 c = f32x2{cur.y, cur.x} * pv;          // (Q Ip, I Qp)
    re = d.x + d.y;
    im = c.x - c.y;
}

}  // namespace sdrk
