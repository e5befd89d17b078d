"""numpy float32 model of the phase discriminator (SDR_FLAG_PHASE_DEMOD, include/sdr_amd.h): this
file is the definition the kernels are tested against, bit for bit.

Every product, sum and quotient below is one numpy float32 operation, so each is rounded on its own
(no FMA), the division is the correctly rounded one, and f32 subnormals are kept.

    re = fl(fl(I Ip) + fl(Q Qp))        im = fl(fl(Q Ip) - fl(I Qp))
    a = |re|, b = |im|, mx = max(a, b), mn = min(a, b);  mx == 0 -> +0
    z = fl(mn / mx),  u = fl(z z)
    p = c_K;  p = fl(fl(p u) + c_k), k = K-1 .. 0;  r = fl(p z)
    b > a -> r = fl(RN32(pi/2) - r);  re < 0 -> r = fl(RN32(pi) - r);  out = copysign(r, im)
"""
from __future__ import annotations

import numpy as np

F = np.float32

# c_0 .. c_K of the odd polynomial atan(z) ~ z (c_0 + c_1 z^2 + .. + c_K z^2K) on [0, 1]; the same hex
# floats as SDR_DEMOD_C* in include/sdr_amd.h (tests/test_demod_model.py compares the two)
COEFFS_HEX = (
    "0x1p+0",
    "-0x1.5550f2p-2",
    "0x1.98d61p-3",
    "-0x1.1e3d8cp-3",
    "0x1.912bfep-4",
    "-0x1.d948p-5",
    "0x1.797d56p-6",
    "-0x1.1d6f96p-8",
)
COEFFS = np.array([float.fromhex(h) for h in COEFFS_HEX], dtype=F)
PI_2 = F(np.pi / 2)     # RN32(pi/2) = 0x1.921fb6p+0
PI = F(np.pi)           # RN32(pi)   = 0x1.921fb6p+1
BOUND = 2.0 ** -20      # absolute error against f64 atan2 of the same f32 (re, im), in rad


def phase(re, im, coeffs=None):
    """The phase of the f32 pair (re, im): f32 array in [-pi, pi] (RN32(pi) at the ends)."""
    c = COEFFS if coeffs is None else np.asarray(coeffs, dtype=F)
    re = np.asarray(re, dtype=F)
    im = np.asarray(im, dtype=F)
    a = np.abs(re)
    b = np.abs(im)
    mx = np.maximum(a, b)
    mn = np.minimum(a, b)
    zero = mx == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (mn / np.where(zero, F(1), mx)).astype(F)
    u = (z * z).astype(F)
    p = np.full(z.shape, c[-1], dtype=F)
    for k in range(len(c) - 2, -1, -1):
        p = ((p * u).astype(F) + c[k]).astype(F)
    r = (p * z).astype(F)
    r = np.where(b > a, (PI_2 - r).astype(F), r)
    r = np.where(re < 0, (PI - r).astype(F), r)
    r = np.copysign(r, im).astype(F)
    return np.where(zero, F(0), r).astype(F)


def products(I, Q, Ip, Qp):
    """(re, im) of x conj(x_prev), each product and sum its own f32 rounding."""
    I, Q, Ip, Qp = (np.asarray(v, dtype=F) for v in (I, Q, Ip, Qp))
    re = ((I * Ip).astype(F) + (Q * Qp).astype(F)).astype(F)
    im = ((Q * Ip).astype(F) - (I * Qp).astype(F)).astype(F)
    return re, im


def demod(I, Q, prev=(0.0, 0.0), coeffs=None):
    """fm_demod of one block of FIR outputs I, Q ([n] or [nch][n]) with the carried previous sample
    prev = (I, Q) ([2] or [nch][2]); returns (out, new_prev)."""
    I = np.asarray(I, dtype=F)
    Q = np.asarray(Q, dtype=F)
    prev = np.asarray(prev, dtype=F)
    Ip = np.concatenate([prev[..., 0:1], I[..., :-1]], axis=-1)
    Qp = np.concatenate([prev[..., 1:2], Q[..., :-1]], axis=-1)
    re, im = products(I, Q, Ip, Qp)
    return phase(re, im, coeffs), np.stack([I[..., -1], Q[..., -1]], axis=-1)


def sine_disc(I, Q, prev=(0.0, 0.0)):
    """The reference's discriminator (demod.cpp:8-19) in f64, for distortion comparisons only (not
    bit-exact): Im(x conj(x_prev)) / |x|^2, 0 where x = 0."""
    I = np.asarray(I, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    Ip = np.concatenate([[prev[0]], I[:-1]])
    Qp = np.concatenate([[prev[1]], Q[:-1]])
    den = I * I + Q * Q
    num = I * (Q - Qp) - Q * (I - Ip)
    return np.where(den == 0, 0.0, num / np.where(den == 0, 1.0, den))


# ---- the distortion measurement behind DESIGN.md 4a'': an f64 copy of the mode-0 front end
FS_RF, DECIM, NTAPS = 2_400_000.0, 10, 101
FS_IF = FS_RF / DECIM
TONE_SKIP = 300            # IF samples dropped in front of the analysis window (the FIR's start-up)


def tone_iq(dev_khz: float, n_iq: int, tone_hz: float = 1000.0, amp: float = 0.85, noise: float = 0.01,
            seed: int = 7) -> np.ndarray:
    """Interleaved u8 I/Q at 2.4 MS/s of one tone at the given peak deviation, quantised as
    synth.FMMultiplexSource quantises (round(127 v + 128), clipped), Gaussian noise on I and Q."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = np.arange(n_iq, dtype=np.float64)
    # phase of a carrier whose instantaneous deviation is dev sin(2 pi f t)
    ph = -(dev_khz * 1e3 / tone_hz) * np.cos(2.0 * np.pi * tone_hz * n / FS_RF)
    i = amp * np.cos(ph) + noise * rng.standard_normal(n_iq)
    q = amp * np.sin(ph) + noise * rng.standard_normal(n_iq)
    out = np.empty(2 * n_iq, np.uint8)
    out[0::2] = np.clip(np.round(127.0 * i + 128.0), 0, 255).astype(np.uint8)
    out[1::2] = np.clip(np.round(127.0 * q + 128.0), 0, 255).astype(np.uint8)
    return out


def lpf_f64(fs: float = FS_RF, fc: float = 100e3, ntaps: int = NTAPS) -> np.ndarray:
    """The front end's low-pass (filter.cpp:13-29: sinc times sin^2(i pi / ntaps)) in f64."""
    cutoff = fc / (fs / 2.0)
    k = np.arange(ntaps, dtype=np.float64) - (ntaps - 1) / 2.0
    return cutoff * np.sinc(cutoff * k) * np.sin(np.arange(ntaps) * np.pi / ntaps) ** 2


def front_f64(u8: np.ndarray):
    """(I, Q) in f64 at 240 kHz: x = (u8 - 128) / 128, the 101-tap FIR, every 10th output, zero history."""
    x = (u8.astype(np.float64) - 128.0) / 128.0
    h = lpf_f64()
    n_if = (x.size // 2) // DECIM
    return tuple(np.convolve(x[k::2], h)[:n_if * DECIM:DECIM] for k in (0, 1))


def tone_readings(y, tone_hz: float = 1000.0, fs: float = FS_IF) -> dict:
    """Of a discriminator output y (radians per sample): the fundamental's amplitude, HD3 in dB and the
    peak as deviation in kHz, over the whole tone periods after TONE_SKIP samples."""
    y = np.asarray(y, dtype=np.float64)[TONE_SKIP:]
    per = int(round(fs / tone_hz))
    y = y[:(y.size // per) * per]
    n = np.arange(y.size)
    amp = [2.0 * abs(np.dot(y, np.exp(-2j * np.pi * k * tone_hz * n / fs))) / y.size for k in (1, 3)]
    return {"fund": amp[0], "hd3_db": 20.0 * np.log10(amp[1] / amp[0]),
            "peak_khz": float(np.max(np.abs(y))) * fs / (2.0 * np.pi) / 1000.0}
