"""CPU: what the RDS carrier-phase derotator's C ABI (include/sdr_amd.h, sdr_rds_carrier_*), the receiver
engine's sdr_multi_run_rds_carrier (include/sdr_multi_rds.h) and the CLI's --rds-carrier refuse before anything
starts. No case reaches a HIP call; the library's constants and records are the model's."""
from __future__ import annotations

import ctypes as C
import subprocess

import pytest

import rds_carrier_model as cm
import rds_track_model as tm
from conftest import ROOT
from test_multi_refusals import INVALID, Wide, file_opts, tuning, vp
from test_multi_rds_refusals import Rds

EXE = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"
RDS_QUAD = 0x10


@pytest.fixture(scope="module")
def host(pkg):
    pkg.lib()
    h = C.CDLL(str(ROOT / "real-time-sdr_amd" / "libsdr_host.so"))
    h.sdr_multi_run_rds_carrier.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    return h


def test_constants_and_records_are_the_models(pkg):
    o = pkg.rds_carrier_opts()
    assert dict(qshift=o.qshift, avg_shift=o.avg_shift) == cm.DEFAULTS
    assert (pkg.RDS_CARRIER_W, pkg.RDS_CARRIER_CORDIC_N) == (cm.W, cm.N_CORDIC)
    assert cm.MAX_N == pkg.RDS_TRACK_MAX_N == tm.MAX_N and cm.QSHIFT == tm.QSHIFT
    dt = pkg.rds_carrier_stats_dtype()
    assert dt.names == cm.STATS and dt.itemsize == 40 == cm.STATS_DTYPE.itemsize
    assert [dt.fields[k][1] for k in cm.STATS] == [cm.STATS_DTYPE.fields[k][1] for k in cm.STATS]
    assert pkg.lib().sdr_version() == 3                     # callers detect the stage by symbol
    with pytest.raises(pkg.SdrError):
        pkg.rds_carrier_opts(no_such_option=1)


def test_create_refuses(pkg):
    L, ref = pkg.lib(), C.byref
    h = C.c_void_p(0x1234)
    good = pkg.rds_carrier_opts()
    assert L.sdr_rds_carrier_create(None, 0, 4, 0, ref(good)) == INVALID
    assert L.sdr_rds_carrier_create(ref(h), 0, 4, 0, None) == INVALID and h.value is None     # *out is cleared
    for nch in (0, -1):
        assert L.sdr_rds_carrier_create(ref(h), 0, nch, 0, ref(good)) == INVALID, nch
    for mode in (1, 2, 3, 4, -1):                            # no RDS chain: sdr_rds_mode_ok
        assert L.sdr_rds_carrier_create(ref(h), 0, 4, mode, ref(good)) == INVALID, mode
        assert b"mode" in L.sdr_last_error()
    for bad in (dict(qshift=-1), dict(qshift=16), dict(avg_shift=-1), dict(avg_shift=7)):
        assert L.sdr_rds_carrier_create(ref(h), 0, 4, 0, ref(pkg.rds_carrier_opts(**bad))) == INVALID, bad
        with pytest.raises(ValueError):
            cm.Channel(**bad)
    assert h.value is None
    L.sdr_rds_carrier_opts_default(None)                     # a NULL is ignored


def test_calls_refuse(pkg):
    """Every refusal of sdr_rds_carrier_rotate comes before the handle is looked at, so a stand-in for it
    (zeroed memory, never a derotator) shows them without a GPU."""
    L = pkg.lib()
    assert L.sdr_rds_carrier_destroy(None) == INVALID and L.sdr_rds_carrier_reset(None, None) == INVALID
    assert L.sdr_rds_carrier_stats_read(None, None, None) == INVALID
    stand_in = C.create_string_buffer(256)
    ri, rq, ro = (C.c_float * 8)(), (C.c_float * 8)(), (C.c_float * 8)()
    h, i_, q_, o_ = C.addressof(stand_in), C.addressof(ri), C.addressof(rq), C.addressof(ro)
    assert L.sdr_rds_carrier_stats_read(h, None, None) == INVALID
    call = L.sdr_rds_carrier_rotate
    assert call(None, i_, 8, q_, 8, 8, o_, 8, None) == INVALID
    assert call(h, None, 8, q_, 8, 8, o_, 8, None) == INVALID
    assert call(h, i_, 8, None, 8, 8, o_, 8, None) == INVALID
    assert call(h, i_, 8, q_, 8, 8, None, 8, None) == INVALID
    assert call(h, i_, 7, q_, 8, 8, o_, 8, None) == INVALID and b"stride_i" in L.sdr_last_error()
    assert call(h, i_, 8, q_, 7, 8, o_, 8, None) == INVALID and b"stride_q" in L.sdr_last_error()
    assert call(h, i_, 8, q_, 8, 8, o_, 7, None) == INVALID and b"out_stride" in L.sdr_last_error()
    assert call(h, i_, 8, q_, 8, -1, o_, 8, None) == INVALID
    big = cm.MAX_N + 1
    assert call(h, i_, big, q_, big, big, o_, big, None) == INVALID and b"SDR_RDS_TRACK_MAX_N" in L.sdr_last_error()
    for k in range(3):                                       # not a float pointer, each row in turn
        p = [i_, q_, o_]
        p[k] += 2
        assert call(h, p[0], 8, p[1], 8, 4, p[2], 8, None) == INVALID
    assert bytes(stand_in) == bytes(256) and not any(ro)


def test_run_rds_carrier_refuses(host, pkg):
    ref = C.byref
    o, good, copts = file_opts(), Rds(2, 8), pkg.rds_carrier_opts()
    TRACK, REF = 1, 0
    run = host.sdr_multi_run_rds_carrier
    assert run(ref(o), None, None, None, None, 0, ref(good), REF, None, None, ref(copts), None) == INVALID   # not on the reference clock
    assert run(ref(o), None, None, None, None, 0, None, TRACK, None, None, ref(copts), None) == INVALID      # no decoder
    for clock in (2, -1):
        assert run(ref(o), None, None, None, None, 0, ref(good), clock, None, None, ref(copts), None) == INVALID, clock
    for mode in (1, 2, 3, 4, -1):
        om = file_opts(mode=mode)
        assert run(ref(om), None, None, None, None, 0, ref(good), TRACK, None, None, ref(copts), None) == INVALID, mode
    for bad in (dict(qshift=-1), dict(qshift=16), dict(avg_shift=-1), dict(avg_shift=7)):
        q = pkg.rds_carrier_opts(**bad)
        assert run(ref(o), None, None, None, None, 0, ref(good), TRACK, None, None, ref(q), None) == INVALID, bad
    # the flag is the engine's to set, on the RDS thread's context
    of = file_opts()
    of.flags |= RDS_QUAD
    assert pkg.RDS_QUAD == RDS_QUAD
    assert run(ref(of), None, None, None, None, 0, ref(good), TRACK, None, None, ref(copts), None) == INVALID
    assert run(ref(of), None, None, None, None, 0, ref(good), TRACK, None, None, None, None) == INVALID
    # what the decoding entries refuse stays refused with the derotator
    assert run(None, None, None, None, None, 0, ref(good), TRACK, None, None, ref(copts), None) == INVALID
    assert run(ref(o), None, None, None, None, 0, ref(Rds(6, 8)), TRACK, None, None, ref(copts), None) == INVALID
    assert run(ref(file_opts(nch=0)), None, None, None, None, 0, ref(good), TRACK, None, None, ref(copts), None) == INVALID
    assert run(ref(o), ref(Wide(4, 1, 0, None)), None, None, None, 0, ref(good), TRACK, None, None, ref(copts), None) == INVALID
    assert run(ref(o), None, ref(tuning(nsrc=0)), None, None, 0, ref(good), TRACK, None, None, ref(copts), None) == INVALID
    bad_track = pkg.rds_track_opts(qshift=16)
    assert run(ref(o), None, None, None, None, 0, ref(good), TRACK, ref(bad_track), None, ref(copts), None) == INVALID
    bad_soft = pkg.RdsSoftOpts(2, 8, 7)
    assert run(ref(o), None, None, None, None, 0, ref(good), TRACK, None, ref(bad_soft), ref(copts), None) == INVALID


@pytest.mark.parametrize("args", [
    ["--rds-carrier", "quad"],                                                     # without --rds-decode
    ["--rds-decode", "--rds-carrier", "quad"],                                     # without the tracker
    ["--rds-decode", "--rds-clock", "ref", "--rds-carrier", "quad"],
    ["--rds-decode", "--rds-clock", "track", "--rds-carrier", "fast"],
    ["--rds-decode", "--rds-clock", "track", "--rds-carrier"],
    ["--rds-decode", "--rds-clock", "track", "--rds-carrier", "quad", "--scan"],
    ["--rds-decode", "--rds-clock", "track", "--rds-carrier", "quad", "--mode", "1"],
    ["--rds-decode", "--rds-clock", "track", "--rds-carrier", "quad", "--mode", "2"],
    ["--rds-decode", "--rds-clock", "track", "--rds-carrier", "quad", "--mode", "3"],
])
def test_cli_refuses(args, tmp_path):
    assert EXE.exists(), "build with make"
    r = subprocess.run([str(EXE), "2", "--in", "/nonexistent/sdr_multi_rds.u8", "--out", str(tmp_path / "rx"), *args],
                       capture_output=True, text=True, timeout=30)
    assert r.returncode == 1 and r.stderr.startswith("usage: sdr_multi"), r.stderr
    assert "--rds-carrier" in r.stderr and not list(tmp_path.iterdir())
