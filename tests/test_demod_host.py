"""CPU: the host-only parts of the phase discriminator's interface (include/sdr_amd.h): the coefficients
the library returns, sdr_meter_deviation, and the refusals of SDR_FLAG_FAST_FRONTEND | SDR_FLAG_PHASE_DEMOD
by sdr_ctx_create, the engine and the CLI -- all before any HIP call."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np

import demod_model as dm
from conftest import ROOT
from test_multi_refusals import INVALID, MISSING, Opts


def test_library_coefficients_are_the_models(pkg):
    c = pkg.demod_coeffs()
    assert c.dtype == np.float32 and np.array_equal(c.view(np.uint32), dm.COEFFS.view(np.uint32))
    n = C.c_int(0)
    assert pkg.lib().sdr_demod_coeffs(None, 0, C.byref(n)) == 0 and n.value == len(dm.COEFFS)
    short = np.full(4, 9.0, np.float32)                 # too little room: only the count comes back
    assert pkg.lib().sdr_demod_coeffs(short.ctypes.data_as(C.c_void_p), 4, C.byref(n)) == 0
    assert np.all(short == 9.0) and n.value == len(dm.COEFFS)


def test_meter_deviation(pkg):
    """peak, rms and offset in kHz are fm_peak, sqrt(fm_sq / n) and fm_sum / n times if_Fs / (2 pi 1000)."""
    for mode, if_fs, n in ((0, 240e3, 7350), (1, 360e3, 13230), (3, 384e3, 12800)):
        row = pkg.MeterRow()
        row.fm_peak, row.fm_sq, row.fm_sum = 1.9634954, 0.5 * n, -0.01 * n
        d = pkg.meter_deviation(mode, row)
        k = if_fs / (2.0 * np.pi) / 1000.0
        want = (k * float(np.float32(1.9634954)), k * np.sqrt(0.5), k * -0.01)
        assert np.allclose([d["peak_khz"], d["rms_khz"], d["offset_khz"]], want, rtol=1e-6, atol=0), (mode, d)
    assert abs(float(pkg.meter_deviation(0, row)["peak_khz"]) - 75.0) < 1e-3      # 2 pi 75 / 240 rad
    assert pkg.lib().sdr_meter_deviation(7, C.byref(row), None, None, None) == INVALID
    assert pkg.lib().sdr_meter_deviation(0, None, None, None, None) == INVALID


def test_fast_and_phase_are_refused(pkg):
    both = pkg.FLAG_FAST_FRONTEND | pkg.PHASE_DEMOD
    h = C.c_void_p()
    assert pkg.lib().sdr_ctx_create(C.byref(h), 0, 2, 0, 1, both) == INVALID and not h.value
    host = C.CDLL(str(ROOT / "real-time-sdr_amd" / "libsdr_host.so"))
    host.sdr_multi_run.argtypes = [C.c_void_p, C.c_void_p]
    o = Opts(nch=3, mode=0, flags=both, in_path=MISSING)
    assert host.sdr_multi_run(C.byref(o), None) == INVALID
    exe = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"
    for args in (["--fast", "--demod", "phase"], ["--demod", "phase", "--fast"], ["--demod", "sine"], ["--demod"]):
        r = subprocess.run([str(exe), "3", "--in", MISSING.decode(), *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stderr.startswith("usage:"), (args, r.stderr)
