"""CPU: what the RDS symbol tracker's C ABI (include/sdr_amd.h, sdr_rds_track_*), the receiver engine's
sdr_multi_run_rds_clock (include/sdr_multi_rds.h) and the CLI's --rds-clock refuse before anything starts. No
case reaches a HIP call; the library's constants and records are the model's."""
from __future__ import annotations

import ctypes as C
import subprocess

import pytest

import rds_track_model as tm
from conftest import ROOT
from test_multi_refusals import INVALID, Wide, file_opts, tuning, vp
from test_multi_rds_refusals import Rds

EXE = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"


@pytest.fixture(scope="module")
def host(pkg):
    pkg.lib()
    h = C.CDLL(str(ROOT / "real-time-sdr_amd" / "libsdr_host.so"))
    h.sdr_multi_run_rds_clock.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp]
    return h


def test_constants_and_records_are_the_models(pkg):
    o = pkg.rds_track_opts()
    assert dict(qshift=o.qshift, acquire_bits=o.acquire_bits, half_bits=o.half_bits) == tm.DEFAULTS
    assert (pkg.RDS_TRACK_T, pkg.RDS_TRACK_CARRY, pkg.RDS_TRACK_MAX_N) == (tm.T, tm.CARRY, tm.MAX_N)
    assert pkg.rds_track_stats_dtype().names == tm.STATS and pkg.rds_track_stats_dtype().itemsize == 32 == tm.STATS_DTYPE.itemsize
    assert pkg.SDR_NBITS_POISONED == tm.NBITS_POISONED and pkg.SDR_MAX_BITS == tm.MAX_BITS
    assert pkg.lib().sdr_version() == 3                     # callers detect the stage by symbol
    with pytest.raises(pkg.SdrError):
        pkg.rds_track_opts(no_such_option=1)


def test_create_refuses(pkg):
    L, ref = pkg.lib(), C.byref
    h = C.c_void_p(0x1234)
    good = pkg.rds_track_opts()
    assert L.sdr_rds_track_create(None, 0, 4, 0, ref(good)) == INVALID
    assert L.sdr_rds_track_create(ref(h), 0, 4, 0, None) == INVALID and h.value is None     # *out is cleared
    for nch in (0, -1):
        assert L.sdr_rds_track_create(ref(h), 0, nch, 0, ref(good)) == INVALID, nch
    for mode in (1, 2, 3, 4, -1):                            # no 1187.5 bit/s clock: sdr_rds_mode_ok
        assert L.sdr_rds_track_create(ref(h), 0, 4, mode, ref(good)) == INVALID, mode
        assert b"mode" in L.sdr_last_error()
    for bad in (dict(qshift=-1), dict(qshift=16), dict(acquire_bits=0), dict(acquire_bits=65), dict(half_bits=0),
                dict(half_bits=8), dict(half_bits=40), dict(half_bits=80)):
        assert L.sdr_rds_track_create(ref(h), 0, 4, 0, ref(pkg.rds_track_opts(**bad))) == INVALID, bad
        with pytest.raises(ValueError):
            tm.Channel(**bad)
    assert h.value is None
    L.sdr_rds_track_opts_default(None)                       # a NULL is ignored


def test_calls_refuse(pkg):
    """Every refusal of sdr_rds_track_bits comes before the handle is looked at, so a stand-in for it (zeroed
    memory, never a tracker) shows them without a GPU."""
    L = pkg.lib()
    assert L.sdr_rds_track_destroy(None) == INVALID and L.sdr_rds_track_reset(None, None) == INVALID
    assert L.sdr_rds_track_stats_read(None, None, None) == INVALID
    stand_in = C.create_string_buffer(256)
    row, nb, bits = (C.c_float * 8)(), (C.c_int32 * 1)(), (C.c_uint8 * 256)()
    t, x, n_, b_ = C.addressof(stand_in), C.addressof(row), C.addressof(nb), C.addressof(bits)
    assert L.sdr_rds_track_stats_read(t, None, None) == INVALID
    call = L.sdr_rds_track_bits
    assert call(None, x, 8, 8, n_, b_, 256, None) == INVALID
    assert call(t, None, 8, 8, n_, b_, 256, None) == INVALID
    assert call(t, x, 8, 8, None, b_, 256, None) == INVALID
    assert call(t, x, 8, 8, n_, None, 256, None) == INVALID
    assert call(t, x, 7, 8, n_, b_, 256, None) == INVALID and b"clean_stride" in L.sdr_last_error()
    assert call(t, x, 8, 8, n_, b_, 255, None) == INVALID and b"bits_stride" in L.sdr_last_error()
    assert call(t, x, 8, -1, n_, b_, 256, None) == INVALID
    assert call(t, x, tm.MAX_N + 1, tm.MAX_N + 1, n_, b_, 256, None) == INVALID and b"SDR_MAX_BITS" in L.sdr_last_error()
    assert call(t, x + 2, 8, 4, n_, b_, 256, None) == INVALID          # not a float pointer
    assert bytes(stand_in) == bytes(256) and nb[0] == 0


def test_run_rds_clock_refuses(host, pkg):
    ref = C.byref
    o, good, topts = file_opts(), Rds(2, 8), pkg.rds_track_opts()
    TRACK, REF = 1, 0
    assert host.sdr_multi_run_rds_clock(ref(o), None, None, None, None, 0, None, TRACK, None, None) == INVALID   # no decoder
    assert host.sdr_multi_run_rds_clock(ref(o), None, None, None, None, 0, None, TRACK, ref(topts), None) == INVALID
    for clock in (2, -1, 7):
        assert host.sdr_multi_run_rds_clock(ref(o), None, None, None, None, 0, ref(good), clock, None, None) == INVALID, clock
    for mode in (1, 2, 3, 4, -1):
        om = file_opts(mode=mode)
        assert host.sdr_multi_run_rds_clock(ref(om), None, None, None, None, 0, ref(good), TRACK, None, None) == INVALID, mode
    for bad in (dict(qshift=16), dict(acquire_bits=0), dict(acquire_bits=65), dict(half_bits=8), dict(half_bits=72)):
        t = pkg.rds_track_opts(**bad)
        assert host.sdr_multi_run_rds_clock(ref(o), None, None, None, None, 0, ref(good), TRACK, ref(t), None) == INVALID, bad
    # what the decoding entry refuses stays refused on either clock
    for clock in (REF, TRACK):
        assert host.sdr_multi_run_rds_clock(None, None, None, None, None, 0, ref(good), clock, None, None) == INVALID
        assert host.sdr_multi_run_rds_clock(ref(o), None, None, None, None, 0, ref(Rds(6, 8)), clock, None, None) == INVALID
        assert host.sdr_multi_run_rds_clock(ref(file_opts(nch=0)), None, None, None, None, 0, ref(good), clock, None, None) == INVALID
        assert host.sdr_multi_run_rds_clock(ref(o), ref(Wide(4, 1, 0, None)), None, None, None, 0, ref(good), clock, None,
                                            None) == INVALID                                     # wide, untuned
        assert host.sdr_multi_run_rds_clock(ref(o), None, ref(tuning(nsrc=0)), None, None, 0, ref(good), clock, None,
                                            None) == INVALID


@pytest.mark.parametrize("args", [
    ["--rds-clock", "track"],                                 # without --rds-decode
    ["--rds-clock", "ref"],
    ["--rds-decode", "--rds-clock", "fast"],
    ["--rds-decode", "--rds-clock"],
    ["--rds-decode", "--rds-clock", "track", "--mode", "1"],
    ["--rds-decode", "--rds-clock", "track", "--mode", "2"],
    ["--rds-decode", "--rds-clock", "track", "--mode", "3"],
    ["--rds-decode", "--rds-clock", "track", "--scan"],
])
def test_cli_refuses(args, tmp_path):
    assert EXE.exists(), "build with make"
    r = subprocess.run([str(EXE), "2", "--in", "/nonexistent/sdr_multi_rds.u8", "--out", str(tmp_path / "rx"), *args],
                       capture_output=True, text=True, timeout=30)
    assert r.returncode == 1 and r.stderr.startswith("usage: sdr_multi"), r.stderr
    assert "--rds-clock" in r.stderr and not list(tmp_path.iterdir())
