"""CPU: what the RF meter's interface refuses before any HIP call (include/sdr_amd.h, SDR_FLAG_IF_ENVELOPE /
sdr_meter_rf*; include/sdr_multi_meter.h): NULL arguments to every new call, the flag with
SDR_FLAG_FAST_FRONTEND in sdr_ctx_create, the engine's validate() cases, and the CLI's usage errors."""
from __future__ import annotations

import ctypes as C
import subprocess

from conftest import ROOT
from test_multi_refusals import INVALID, MISSING, Opts, Wide, entries, file_opts, host, tuning  # noqa: F401 (host: a fixture)


def test_null_arguments(pkg):
    L = pkg.lib()
    row, o, st = pkg.MeterRfRow(), pkg.meter_rf_opts(), pkg.MeterRfState()
    one = C.c_void_p(1 << 12)                       # never dereferenced: the other argument is NULL
    assert L.sdr_meter_rf(None, one, None) == INVALID
    assert L.sdr_meter_rf(one, None, None) == INVALID
    assert L.sdr_meter_rf(None, None, None) == INVALID
    assert L.sdr_meter_rf_read(None, one, None) == INVALID
    assert L.sdr_meter_rf_rows(None, C.byref(C.c_void_p())) == INVALID
    assert L.sdr_meter_rf_status(0, None, C.byref(o), C.byref(st)) == INVALID
    assert L.sdr_meter_rf_status(0, C.byref(row), None, C.byref(st)) == INVALID
    assert L.sdr_meter_rf_status(0, C.byref(row), C.byref(o), None) == INVALID
    for mode in (-1, 4):
        assert L.sdr_meter_rf_status(mode, C.byref(row), C.byref(o), C.byref(st)) == INVALID
    L.sdr_meter_rf_opts_default(None)               # returns
    assert pkg.IF_ENVELOPE == 0x20 and C.sizeof(pkg.MeterRfRow) == 32


def test_fast_and_envelope_are_refused_by_ctx_create(pkg):
    for extra in (0, pkg.PHASE_DEMOD, pkg.FLAG_KEEP_INTERMEDIATES):
        h = C.c_void_p()
        flags = pkg.FLAG_FAST_FRONTEND | pkg.IF_ENVELOPE | extra
        assert pkg.lib().sdr_ctx_create(C.byref(h), 0, 2, 0, 1, flags) == INVALID and not h.value
        assert b"SDR_FLAG" in pkg.lib().sdr_last_error()


def test_engine_refuses_the_flag_without_a_meter_or_with_fast(host, pkg):
    """validate(): SDR_FLAG_IF_ENVELOPE needs a meter and the exact front end, through every entry point."""
    mo, ao, t, w = pkg.meter_opts(), pkg.audio_opts(), tuning(), Wide(4, 1, 0, None)
    ref = C.byref
    env = file_opts(flags=pkg.IF_ENVELOPE)
    fast = file_opts(flags=pkg.IF_ENVELOPE | pkg.FLAG_FAST_FRONTEND)
    # no meter
    assert host.sdr_multi_run(ref(env), None) == INVALID
    assert host.sdr_multi_run_tuned(ref(env), ref(t), None) == INVALID
    assert host.sdr_multi_run_tuned(ref(env), None, None) == INVALID
    assert host.sdr_multi_run_metered(ref(env), None, None, None) == INVALID
    assert host.sdr_multi_run_finished(ref(env), None, None, ref(ao), 0, None) == INVALID
    assert host.sdr_multi_run_wide(ref(env), ref(w), ref(t), None, ref(ao), 0, None) == INVALID
    # a meter, but the MFMA front end
    for name, f in entries(host, pkg).items():
        assert f(ref(fast)) == INVALID, name


def test_cli_usage_errors():
    exe = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"
    for args in (["--rf"], ["--rf", "--deemph", "75"], ["--meter", "--rf", "--fast"], ["--fast", "--rf", "--meter"],
                 ["--scan", "--rf"]):
        r = subprocess.run([str(exe), "3", "--in", MISSING.decode(), *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stderr.startswith("usage:"), (args, r.stderr)
        assert "[--meter [--rf]]" in r.stderr and "--rf: also write PREFIX.rf" in r.stderr
