"""CPU: the audio finishing stage's host side (include/sdr_amd.h: sdr_audio_coeffs, the defaults, the
refusals that need no GPU) and the properties of its model (tests/audio_model.py) that the GPU tests
build on: identity, the decay through f32 subnormals, the frequency response, the blend map. No GPU is
touched."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import audio_model as am
import meter_model as mm
from conftest import ROOT

N = am.N_AUDIO


# ---------------------------------------------------------------- the C ABI without a device
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_coeffs_equal_the_model(pkg, mode):
    for tau in (50.0, 75.0):
        a, b = pkg.audio_coeffs(mode, tau)
        wa, wb = am.coeffs(mode, tau)
        assert a.view(np.uint32) == wa.view(np.uint32) and b.view(np.uint32) == wb.view(np.uint32), (mode, tau, a, wa)
        assert 0.6 < a < 0.78 and b == np.float32(1.0 - float(a))
    assert pkg.audio_coeffs(mode, 0.0) == (0.0, 1.0)


def test_coeff_values(pkg):
    assert abs(float(pkg.audio_coeffs(0, 75.0)[0]) - 0.7574651) < 1e-7
    assert abs(float(pkg.audio_coeffs(0, 50.0)[0]) - 0.6592406) < 1e-7
    assert abs(float(pkg.audio_coeffs(1, 75.0)[0]) - 0.7165313) < 1e-7


def test_defaults_layout_and_version(pkg):
    o = pkg.audio_opts()
    assert (o.tau_us, o.blend_lo, o.blend_hi) == (75.0, 0.5, 2.0)
    assert C.sizeof(pkg.AudioState) == 24 and am.STATE_DTYPE.itemsize == 24
    assert pkg.audio_state_dtype().itemsize == 24
    for name in am.STATE_DTYPE.names:
        assert am.STATE_DTYPE.fields[name][1] == getattr(pkg.AudioState, name).offset, name
    assert pkg.lib().sdr_version() == 3          # the stage is detected by symbol, not by version
    pkg.lib().sdr_audio_opts_default(None)       # tolerated, like the meter's
    with pytest.raises(pkg.SdrError):
        pkg.audio_opts(no_such_option=1)


def test_refusals_without_a_gpu(pkg):
    L = pkg.lib()
    vp = C.c_void_p
    a, b = C.c_float(), C.c_float()
    assert L.sdr_audio_coeffs(4, 75.0, C.byref(a), C.byref(b)) == -1
    assert L.sdr_audio_coeffs(-1, 75.0, C.byref(a), C.byref(b)) == -1
    assert L.sdr_audio_coeffs(0, 75.0, None, C.byref(b)) == -1
    assert L.sdr_audio_coeffs(0, 75.0, C.byref(a), None) == -1
    for tau in (-1.0, math.nan, math.inf, 1000.5):
        assert L.sdr_audio_coeffs(0, tau, C.byref(a), C.byref(b)) == -1, tau
    assert L.sdr_audio_coeffs(0, 1000.0, C.byref(a), C.byref(b)) == 0

    h = vp()
    good = pkg.audio_opts()
    assert L.sdr_audio_create(None, 0, 1, 0, 2, C.byref(good)) == -1
    assert L.sdr_audio_create(C.byref(h), 0, 1, 0, 2, None) == -1 and not h.value
    assert L.sdr_audio_create(C.byref(h), 0, 1, 7, 2, C.byref(good)) == -1 and not h.value       # bad mode
    assert L.sdr_audio_create(C.byref(h), 0, 0, 0, 2, C.byref(good)) == -1 and not h.value       # nch < 1
    for width in (0, 3):
        assert L.sdr_audio_create(C.byref(h), 0, 1, 0, width, C.byref(good)) == -1 and not h.value
    for bad in (dict(tau_us=-1.0), dict(tau_us=math.nan), dict(tau_us=math.inf), dict(tau_us=1001.0),
                dict(blend_lo=2.0), dict(blend_lo=1.0, blend_hi=0.5), dict(blend_hi=math.nan)):
        o = pkg.audio_opts(**bad)
        assert L.sdr_audio_create(C.byref(h), 0, 1, 0, 2, C.byref(o)) == -1 and not h.value, bad
    assert L.sdr_audio_destroy(None) == -1
    assert L.sdr_audio_reset(None, None) == -1
    assert L.sdr_audio_set_control(None, None, None, None) == -1
    assert L.sdr_audio_blend_from_meter(None, None, None) == -1
    assert L.sdr_audio_finish(None, None, 0, None, 0, None) == -1
    assert L.sdr_audio_read_state(None, None, None) == -1

    host = C.CDLL(str(ROOT / "real-time-sdr_amd" / "libsdr_host.so"))
    fn = host.sdr_multi_run_finished
    fn.argtypes = [vp, vp, vp, vp, C.c_int, vp]
    opts = (C.c_char * 1024)()                      # zeroed sdr_multi_opts: never read past the checks below
    mo = pkg.meter_opts()
    assert fn(None, None, None, C.byref(good), 0, None) == -1
    assert fn(opts, None, None, None, 0, None) == -1                         # no audio options
    assert fn(opts, None, None, C.byref(good), 1, None) == -1                # blend without a meter
    badtau = pkg.audio_opts(tau_us=-5.0)
    assert fn(opts, None, C.byref(mo), C.byref(badtau), 1, None) == -1


# ---------------------------------------------------------------- the model's own properties
def test_model_identity():
    """tau 0, blend 1, gain 1: the samples come back, except that -32768 becomes -32767."""
    rs = np.random.Generator(np.random.PCG64(3))
    x = rs.integers(-32768, 32768, (4, 2 * N), dtype=np.int16)
    x[0, :16] = -32768
    x[1, 5] = x[1, 6] = 32767
    m = am.AudioFinish(4, tau_us=0.0)
    for _ in range(2):
        y = m.finish(x)
        assert np.array_equal(y, np.maximum(x, -32767))
    m1 = am.AudioFinish(4, width=1, n=2 * N, tau_us=0.0)
    assert np.array_equal(m1.finish(x), np.maximum(x, -32767))


def impulse_rows():
    x = np.zeros((1, 2 * N), np.int16)
    x[0, 0], x[0, 1] = 32767, -20000
    return x


def test_model_decay_passes_through_subnormals():
    """75 us at 48 kHz: within one block the impulse response falls below the smallest normal f32 and
    settles at +-2 denormal steps (a * 2 ulp rounds back to 2 ulp), not at 0 -- what a flushing build
    could not reproduce."""
    m = am.AudioFinish(1)
    m.finish(impulse_rows())
    y = m.state()["y"][0]
    tiny = np.finfo(np.float32).tiny
    step = np.float32(2.0 ** -149)
    assert y[0] == 2 * step and y[1] == -2 * step, y
    assert 0 < abs(y[0]) < tiny and 0 < abs(y[1]) < tiny
    out = m.finish(np.zeros((1, 2 * N), np.int16))
    assert not out.any()
    assert np.array_equal(m.state()["y"][0].view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("mode,tau", [(0, 75.0), (0, 50.0), (1, 75.0), (2, 50.0)])
def test_model_frequency_response(mode, tau):
    """A 16000-amplitude sine over three blocks, measured on blocks 2-3: within 0.01 dB of the one-pole's
    |b / (1 - a e^{-jw})| (output rounding bounds the error near 0.002 dB at 15 kHz)."""
    fs = am.FS_AUDIO[mode]
    a, b = am.coeffs(mode, tau)
    freqs = (1000.0, 5000.0, 10000.0, 15000.0)
    t = np.arange(3 * N) / fs
    x = np.stack([np.rint(16000.0 * np.sin(2 * np.pi * f * t)) for f in freqs]).astype(np.int16)   # [freq][3 N]
    m = am.AudioFinish(len(freqs), mode=mode, width=1, tau_us=tau)
    y = np.concatenate([m.finish(x[:, k * N:(k + 1) * N]) for k in range(3)], axis=1).astype(np.float64)
    for i, f in enumerate(freqs):
        basis = np.stack([np.cos(2 * np.pi * f * t[N:]), np.sin(2 * np.pi * f * t[N:])], axis=1)
        amp = [np.hypot(*np.linalg.lstsq(basis, v[i, N:], rcond=None)[0]) for v in (y, x.astype(np.float64))]
        gain = amp[0] / amp[1]
        err_db = 20 * math.log10(gain / am.response(a, b, f, fs))
        print(f"mode {mode} tau {tau} f {f}: {20 * math.log10(gain):.4f} dB, error {err_db:+.5f} dB")
        assert abs(err_db) <= 0.01, (f, err_db)


def _row(**f):
    r = np.zeros((), mm.ROW_DTYPE)
    for k, v in f.items():
        r[k] = v
    return r


def test_blend_map_on_hand_made_rows():
    noise = np.float32(3.0)
    rows, want = [], []
    for k, g in ((0.5, 0.0), (1.25, 0.5), (2.0, 1.0), (3.0, 1.0), (0.25, 0.0)):
        rows.append(_row(flags=1, pilot_sq=np.float32(k) * noise * np.float32(5), noise_sq=noise))   # P / Z = k
        want.append(g)
    rows += [_row(flags=1, pilot_sq=0.0, noise_sq=1.0), _row(flags=3, pilot_sq=1e-3, noise_sq=0.0),
             _row(flags=1, pilot_sq=np.nan, noise_sq=np.nan), _row(flags=1, pilot_sq=1.0, noise_sq=np.nan),
             _row(flags=1, pilot_sq=np.inf, noise_sq=np.inf), _row(flags=2, pilot_sq=100.0, noise_sq=1.0),
             _row(flags=0, pilot_sq=0.0, noise_sq=1.0)]
    want += [0.0, 1.0, 0.0, 0.0, 0.0, 0.25, 0.25]                # the last two: no AUDIO flag, unchanged
    got = am.blend_map(np.stack(rows), np.float32(0.25))
    assert got.dtype == np.float32 and np.array_equal(got, np.array(want, np.float32)), got
    # other corners
    got = am.blend_map(np.stack(rows[:4]), np.float32(1), lo=1.0, hi=3.0)
    assert np.array_equal(got, np.array([0.0, 0.125, 0.5, 1.0], np.float32)), got


def test_blend_map_on_the_kinds(oracle, synth):
    """The model's meter rows of synth.KINDS (CPU-made bytes, blocks 6-9): exactly 1 with a pilot,
    exactly 0 without."""
    import torch
    kinds = ("normal", "pilot_offset", "carrier_offset", "no_pilot", "noise", "silence")
    gen = synth.TorchMultiplexBatch(torch, len(synth.KINDS), 0, "cpu", kinds=synth.KINDS, seed=11)
    blocks = np.stack([gen.next_block().numpy().copy() for _ in range(10)])
    for kind in kinds:
        rows = mm.run_rows(oracle, 0, blocks[:, synth.KINDS.index(kind)])
        for b in range(6, 10):
            g = am.blend_map(rows[b], np.float32(0.5))[0]
            assert g == (1.0 if kind in kinds[:3] else 0.0), (kind, b, g)
