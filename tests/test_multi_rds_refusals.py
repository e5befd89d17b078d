"""CPU: what the receiver engine's decoding entry point (include/sdr_multi_rds.h, sdr_multi_run_rds) and the
CLI's --rds-decode / --rds-correct refuse before anything starts. No case reaches a HIP call."""
from __future__ import annotations

import ctypes as C
import subprocess

import pytest

from conftest import ROOT
from test_multi_refusals import INVALID, Opts, Wide, file_opts, tuning, vp

EXE = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"


class Rds(C.Structure):                         # sdr_multi_rds (include/sdr_multi_rds.h)
    _fields_ = [("max_burst", C.c_int), ("loss_blocks", C.c_int)]


@pytest.fixture(scope="module")
def host(pkg):
    pkg.lib()
    h = C.CDLL(str(ROOT / "real-time-sdr_amd" / "libsdr_host.so"))
    h.sdr_multi_run_rds.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp]
    return h


def test_mode_ok(pkg):
    L = pkg.lib()
    assert [L.sdr_rds_mode_ok(m) for m in (-1, 0, 1, 2, 3, 4)] == [0, 1, 0, 0, 0, 0]


def test_run_rds_refuses(host, pkg):
    ref = C.byref
    mo, ao, t, w = pkg.meter_opts(), pkg.audio_opts(), tuning(), Wide(4, 1, 0, None)
    good = Rds(2, 8)
    o = file_opts()
    for bad in (Rds(-1, 8), Rds(6, 8), Rds(2, 0), Rds(2, 65), Rds(2, -3)):
        assert host.sdr_multi_run_rds(ref(o), None, None, None, None, 0, ref(bad), None) == INVALID, (bad.max_burst, bad.loss_blocks)
        assert host.sdr_multi_run_rds(ref(o), ref(w), ref(t), ref(mo), ref(ao), 1, ref(bad), None) == INVALID
    for mode in (1, 2, 3, 4, -1):                                      # no RDS bit clock in the mode
        om = file_opts(mode=mode)
        assert host.sdr_multi_run_rds(ref(om), None, None, None, None, 0, ref(good), None) == INVALID, mode
    # what the other entries refuse stays refused with the decoder
    assert host.sdr_multi_run_rds(None, None, None, None, None, 0, ref(good), None) == INVALID
    for nch in (0, -2):
        on = file_opts(nch=nch)
        assert host.sdr_multi_run_rds(ref(on), None, None, None, None, 0, ref(good), None) == INVALID
    assert host.sdr_multi_run_rds(ref(o), ref(w), None, None, None, 0, ref(good), None) == INVALID        # wide, untuned
    assert host.sdr_multi_run_rds(ref(o), None, None, None, ref(ao), 1, ref(good), None) == INVALID       # blend, no meter
    assert host.sdr_multi_run_rds(ref(o), None, ref(tuning(nsrc=0)), None, None, 0, ref(good), None) == INVALID
    flags = file_opts(flags=0x1 | 0x8)                                 # fast front end with the phase discriminator
    assert host.sdr_multi_run_rds(ref(flags), None, None, None, None, 0, ref(good), None) == INVALID
    # without the decoder it is sdr_multi_run_wide
    assert host.sdr_multi_run_rds(None, None, None, None, None, 0, None, None) == INVALID


@pytest.mark.parametrize("args", [
    ["--rds-correct", "2"],                         # without --rds-decode
    ["--rds-decode", "--rds-correct", "6"],
    ["--rds-decode", "--rds-correct", "-1"],
    ["--rds-decode", "--rds-correct", "two"],
    ["--rds-decode", "--rds-correct"],
    ["--rds-decode", "--mode", "1"],
    ["--rds-decode", "--mode", "2"],
    ["--rds-decode", "--mode", "3"],
    ["--rds-decode", "--scan"],
])
def test_cli_refuses(args, tmp_path):
    assert EXE.exists(), "build with make"
    r = subprocess.run([str(EXE), "2", "--in", "/nonexistent/sdr_multi_rds.u8", "--out", str(tmp_path / "rx"), *args],
                       capture_output=True, text=True, timeout=30)
    assert r.returncode == 1 and r.stderr.startswith("usage: sdr_multi"), r.stderr
    assert "--rds-decode" in r.stderr and not list(tmp_path.iterdir())
