"""CPU model of the audio finishing stage (include/sdr_amd.h, sdr_audio_*): de-emphasis, the stereo
blend and the gain, with np.float32 at every rounding -- vectorised over the channels, a loop over the
frames -- the poison rule, and the blend-from-meter map over meter_model.ROW_DTYPE rows. Every output
sample and every state float is meant to equal the GPU's bit for bit."""
from __future__ import annotations

import math

import numpy as np

import meter_model as mm

POISON = -32768
N_AUDIO = 1470
FS_AUDIO = {0: 48000.0, 1: 40000.0, 2: 44100.0, 3: 44100.0}      # if_Fs * U / D
DEFAULTS = dict(tau_us=75.0, blend_lo=0.5, blend_hi=2.0)
STATE_DTYPE = np.dtype([("y", "<f4", (2,)), ("blend", "<f4"), ("gain", "<f4"), ("blend_target", "<f4"),
                        ("gain_target", "<f4")])
f32 = np.float32


def coeffs(mode: int, tau_us: float):
    """(a, b) as float32: a = RN32(exp(-1e6 / (tau_us Fs_a))), b = RN32(1 - a), both from double."""
    if tau_us == 0:
        return f32(0), f32(1)
    a = f32(math.exp(-1e6 / (float(f32(tau_us)) * FS_AUDIO[mode])))
    return a, f32(1.0 - float(a))


def response(a, b, f_hz, fs):
    """|b / (1 - a e^{-jw})| of the one-pole, in double."""
    w = 2.0 * math.pi * f_hz / fs
    return float(b) / abs(1.0 - float(a) * np.exp(-1j * w))


def blend_map(rows, current, mode: int = 0, lo=0.5, hi=2.0):
    """sdr_audio_blend_from_meter: the new blend targets [nch] from the meter rows [nch]; a row without
    the AUDIO flag keeps `current`."""
    rows = np.atleast_1d(np.asarray(rows, mm.ROW_DTYPE))
    out = np.array(np.broadcast_to(np.asarray(current, f32), rows.shape), f32)
    n, q = f32(mm.BLOCK_IF[mode]), f32(mm.BLOCK_IF[mode] // 5)
    lo, span = f32(lo), f32(f32(hi) - f32(lo))
    with np.errstate(all="ignore"):
        for i, r in enumerate(rows):
            if not int(r["flags"]) & mm.ROW_AUDIO:
                continue
            P, Z = f32(r["pilot_sq"] * q), f32(r["noise_sq"] * n)
            if not P > 0:
                g = f32(0)
            elif Z == 0:
                g = f32(1)
            else:
                x = f32(f32(f32(P / Z) - lo) / span)
                g = f32(0) if not x > 0 else (f32(1) if x > 1 else x)
            out[i] = g
    return out


class AudioFinish:
    """The model of `nch` channels: set_control / blend_from_meter, then finish(block) per block."""

    def __init__(self, nch: int, mode: int = 0, width: int = 2, n: int = N_AUDIO, **opts):
        o = dict(DEFAULTS, **opts)
        self.nch, self.mode, self.width, self.n = nch, mode, width, n
        self.a, self.b = coeffs(mode, o["tau_us"])
        self.lo, self.hi = o["blend_lo"], o["blend_hi"]
        self.reset()

    def reset(self):
        self.y = np.zeros((self.nch, 2), f32)
        self.g0, self.g1, self.v0, self.v1 = (np.ones(self.nch, f32) for _ in range(4))

    def set_control(self, blend=None, gain=None):
        if blend is not None:
            self.g1 = np.array(np.broadcast_to(np.asarray(blend, f32), (self.nch,)), f32)
        if gain is not None:
            self.v1 = np.array(np.broadcast_to(np.asarray(gain, f32), (self.nch,)), f32)

    def blend_from_meter(self, rows):
        self.g1 = blend_map(rows, self.g1, self.mode, self.lo, self.hi)

    def state(self):
        s = np.zeros(self.nch, STATE_DTYPE)
        s["y"], s["blend"], s["gain"], s["blend_target"], s["gain_target"] = self.y, self.g0, self.v0, self.g1, self.v1
        return s

    def finish(self, block):
        """block: int16 [nch][>= width * n] (only the first width * n of a row count); returns [nch][width * n]."""
        W, N, a, b = self.width, self.n, self.a, self.b
        x = np.asarray(block)[:, :W * N]
        assert x.dtype == np.int16 and x.shape == (self.nch, W * N)
        pois = (x == POISON).all(axis=1)
        xf = x.astype(f32)
        rN = f32(f32(1.0) / f32(N))
        dg, dv = self.g1 - self.g0, self.v1 - self.v0
        half = f32(0.5)
        out = np.empty((self.nch, W * N), np.int16)
        y = self.y.copy()
        with np.errstate(under="ignore"):
            for n in range(N):
                t = f32(f32(n + 1) * rN)
                v = self.v0 + dv * t
                if W == 2:
                    g = self.g0 + dg * t
                    l, r = xf[:, 2 * n], xf[:, 2 * n + 1]
                    m, s = half * (l + r), half * (l - r)
                    p = g * s
                    xs = (m + p, m - p)
                else:
                    xs = (xf[:, n],)
                for w in range(W):
                    y[:, w] = a * y[:, w] + b * xs[w]
                    out[:, W * n + w] = np.clip(np.rint(v * y[:, w]), -32767, 32767).astype(np.int16)
        assert y.dtype == f32 and dg.dtype == f32
        y[pois] = 0
        out[pois] = POISON
        self.y = y
        self.g0, self.v0 = self.g1.copy(), self.v1.copy()
        return out


def same_state(got, want) -> list:
    """The fields in which two state arrays differ, compared as uint32: [] when equal."""
    bad = []
    for name in STATE_DTYPE.names:
        if not np.array_equal(np.ascontiguousarray(got[name]).view(np.uint32),
                              np.ascontiguousarray(want[name]).view(np.uint32)):
            bad.append(name)
    return bad
