"""CPU: the phase discriminator's definition (tests/demod_model.py, include/sdr_amd.h
SDR_FLAG_PHASE_DEMOD): its accuracy against f64 atan2, its edge cases, and what it does to a loud
tone that the sine discriminator folds (DESIGN.md 4a'')."""
from __future__ import annotations

import re

import numpy as np
import pytest

import demod_model as dm
from conftest import ROOT

F = np.float32


def _err(re_, im_):
    got = dm.phase(re_, im_).astype(np.float64)
    ref = np.arctan2(np.asarray(im_, F).astype(np.float64), np.asarray(re_, F).astype(np.float64))
    return float(np.max(np.abs(got - ref)))


def test_header_coefficients_are_the_models():
    """SDR_DEMOD_C0 .. C7, SDR_DEMOD_PI_2 and SDR_DEMOD_PI of include/sdr_amd.h are the model's values."""
    text = (ROOT / "include" / "sdr_amd.h").read_text()
    k = int(re.search(r"#define SDR_DEMOD_K (\d+)", text).group(1))
    assert k + 1 == len(dm.COEFFS)
    for i in range(k + 1):
        hx = re.search(rf"#define SDR_DEMOD_C{i} (\S+?)f\b", text).group(1)
        assert F(float.fromhex(hx)) == dm.COEFFS[i] and float.fromhex(hx) == float(dm.COEFFS[i]), f"c_{i}"
    for name, want in (("PI_2", dm.PI_2), ("PI", dm.PI)):
        hx = re.search(rf"#define SDR_DEMOD_{name} (\S+?)f\b", text).group(1)
        assert float.fromhex(hx) == float(want), name


def test_accuracy_every_z_in_every_octant():
    """All 2^24 + 1 quotients z = m 2^-24 (mx = 1, mn = z, both exact f32), crossed with which of |re|,
    |im| is the larger and the two signs: at most 2^-20 rad from f64 atan2 of the same pair."""
    worst = 0.0
    step = 1 << 21
    for lo in range(0, (1 << 24) + 1, step):
        m = np.arange(lo, min(lo + step, (1 << 24) + 1), dtype=np.float64)
        z = (m * 2.0 ** -24).astype(F)
        assert np.array_equal(z.astype(np.float64), m * 2.0 ** -24)
        one = np.ones_like(z)
        for a, b in ((one, z), (z, one)):
            for sr in (F(1), F(-1)):
                for si in (F(1), F(-1)):
                    worst = max(worst, _err(a * sr, b * si))
    print(f"max |model - atan2| over the z grid: {worst:.4g} rad = {worst / dm.BOUND:.4f} x 2^-20")
    assert worst <= dm.BOUND


def test_accuracy_random_pairs():
    """10^6 random (re, im) over 40 binades of magnitude and ratio, subnormal quotients included."""
    rng = np.random.default_rng(20)
    n = 1_000_000
    mag = np.exp2(rng.uniform(-20, 20, n))
    ang = rng.uniform(-np.pi, np.pi, n)
    re_ = (mag * np.cos(ang)).astype(F)
    im_ = (mag * np.sin(ang)).astype(F)
    # a quarter of them with a tiny minor component (z down to the subnormals)
    tiny = rng.random(n) < 0.25
    im_ = np.where(tiny, (im_ * np.exp2(rng.uniform(-140, -20, n))).astype(F), im_)
    worst = _err(re_, im_)
    print(f"max |model - atan2| over random pairs: {worst:.4g} rad = {worst / dm.BOUND:.4f} x 2^-20")
    assert worst <= dm.BOUND


def _bits(x):
    return np.asarray(x, F).view(np.uint32)


def test_edge_cases():
    pi, pi_2 = dm.PI, dm.PI_2
    sub = F(1e-45)                                      # the smallest f32 subnormal
    assert sub > 0 and sub < np.finfo(F).tiny
    cases = [
        ((0.0, 0.0), F(0)), ((-0.0, 0.0), F(0)), ((0.0, -0.0), F(0)), ((-0.0, -0.0), F(0)),   # mx == 0 -> +0
        ((-0.0, 1.0), pi_2), ((-0.0, -1.0), -pi_2),     # re = -0 is not < 0
        ((0.0, 1.0), pi_2), ((1.0, 0.0), F(0)), ((1.0, -0.0), F(-0.0)),
        ((-1.0, 0.0), pi), ((-1.0, -0.0), -pi),         # im = +-0 with re < 0: +-pi by im's sign
        ((-sub, 0.0), pi), ((-sub, -0.0), -pi),
        ((sub, sub), None), ((-sub, sub), None), ((sub, -sub), None),                        # a == b, subnormal
        ((1.0, 1.0), None), ((-1.0, 1.0), None), ((-3.5, -3.5), None),                       # a == b
        ((sub, 1.0), pi_2), ((1.0, sub), sub), ((-1.0, sub), pi), ((-1.0, -sub), -pi),       # subnormal minor
    ]
    for (re_, im_), want in cases:
        got = dm.phase(F(re_), F(im_))
        if want is None:                                # equal magnitudes: z = 1, the diagonal
            ref = np.arctan2(np.float64(F(im_)), np.float64(F(re_)))
            assert abs(float(got) - ref) <= dm.BOUND, (re_, im_, got)
            assert not (np.abs(F(im_)) > np.abs(F(re_)))   # b > a is false: no pi/2 reflection
        else:
            assert _bits(got) == _bits(want), (re_, im_, got, want)
    # the diagonal is fl(p(1)) whatever the magnitude
    assert _bits(dm.phase(F(1), F(1))) == _bits(dm.phase(sub, sub)) == _bits(dm.phase(F(3e38), F(3e38)))


def test_small_steps_equal_the_sine_discriminator():
    """For a small step the value is the sine discriminator's (c_0 = 1): levels downstream keep their scale."""
    th = np.linspace(-0.01, 0.01, 2001)
    x = np.exp(1j * np.cumsum(th))
    I, Q = x.real.astype(F), x.imag.astype(F)
    p, prev = dm.demod(I, Q, (1.0, 0.0))
    s = dm.sine_disc(I, Q, (1.0, 0.0))
    assert np.max(np.abs(p.astype(np.float64) - s)) < 2e-6 + 0.01 ** 3      # sin x = x - x^3/6, f32 products
    assert _bits(prev[0]) == _bits(I[-1]) and _bits(prev[1]) == _bits(Q[-1])


def test_demod_carry_and_batch():
    """demod's carried previous sample: two half blocks equal one whole block; rows are independent."""
    rng = np.random.default_rng(3)
    I, Q = (rng.standard_normal((3, 64)).astype(F) for _ in range(2))
    whole, pv = dm.demod(I, Q, np.zeros((3, 2), F))
    a, p1 = dm.demod(I[:, :20], Q[:, :20], np.zeros((3, 2), F))
    b, p2 = dm.demod(I[:, 20:], Q[:, 20:], p1)
    assert np.array_equal(_bits(np.concatenate([a, b], axis=1)), _bits(whole)) and np.array_equal(pv, p2)
    assert np.all(whole[:, 0] == 0)                     # zero carry: mx == 0
    one, _ = dm.demod(I[1], Q[1], np.zeros(2, F))
    assert np.array_equal(_bits(one), _bits(whole[1]))


@pytest.fixture(scope="module")
def tone75():
    """(I, Q) of the 75 kHz-deviation tone through the f64 front end (2 blocks of mode 0)."""
    return dm.front_f64(dm.tone_iq(75.0, 2 * 73500))


def test_tone_75khz_phase_discriminator(tone75):
    """1 kHz at 75 kHz deviation, amplitude 0.85, noise 0.01, u8: the f32 model on the f64 FIR outputs
    rounded to f32. HD3 <= -60 dB, fundamental within 1 % of 2 pi 75 / 240, peak 75 +- 1.5 kHz."""
    I, Q = tone75
    y, _ = dm.demod(I.astype(F), Q.astype(F))
    r = dm.tone_readings(y)
    print(f"phase discriminator: {r}")
    assert r["hd3_db"] <= -60.0
    assert abs(r["fund"] / (2.0 * np.pi * 75.0 / 240.0) - 1.0) <= 0.01
    assert abs(r["peak_khz"] - 75.0) <= 1.5


def test_tone_75khz_sine_discriminator_folds(tone75):
    """The same I/Q through the reference's discriminator: third harmonic above -20 dB."""
    I, Q = tone75
    r = dm.tone_readings(dm.sine_disc(I, Q))
    print(f"sine discriminator: {r}")
    assert r["hd3_db"] > -20.0
