"""CPU: what the RDS soft decisions' C ABI (include/sdr_amd.h, sdr_rds_track_bits_soft and sdr_rds_*_soft), the
receiver engine's sdr_multi_run_rds_soft (include/sdr_multi_rds.h) and the CLI's --rds-soft refuse before
anything starts. No case reaches a HIP call; the library's constants and records are the model's. (A handle of
sdr_rds_dec_create_soft refusing sdr_rds_groups needs such a handle: tests/test_gpu_rds_soft.py.)"""
from __future__ import annotations

import ctypes as C
import subprocess

import pytest

import rds_soft_model as sm
from conftest import ROOT
from test_multi_refusals import INVALID, file_opts, vp
from test_multi_rds_refusals import Rds

EXE = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"
TRACK, REF = 1, 0


@pytest.fixture(scope="module")
def host(pkg):
    pkg.lib()
    h = C.CDLL(str(ROOT / "real-time-sdr_amd" / "libsdr_host.so"))
    h.sdr_multi_run_rds_soft.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    return h


def test_constants_and_records_are_the_models(pkg):
    o = pkg.rds_soft_opts()
    assert dict(max_burst=o.max_burst, loss_blocks=o.loss_blocks, soft_bits=o.soft_bits) == sm.SOFT_DEFAULTS
    assert pkg.rds_soft_stats_dtype().names == sm.SOFT_STATS_DTYPE.names
    assert pkg.rds_soft_stats_dtype().itemsize == 16 == sm.SOFT_STATS_DTYPE.itemsize
    assert (pkg.RDS_GROUP_SOFT_SHIFT, pkg.RDS_SOFT_HISTORY) == (sm.GROUP_SOFT_SHIFT, sm.HIST)
    assert pkg.rds_group_dtype().itemsize == 16 and pkg.rds_stats_dtype().itemsize == 32      # the records did not move
    assert pkg.lib().sdr_version() == 3                     # callers detect the stage by symbol
    with pytest.raises(pkg.SdrError):
        pkg.rds_soft_opts(no_such_option=1)
    pkg.lib().sdr_rds_soft_opts_default(None)               # a NULL is ignored


def test_create_soft_refuses(pkg):
    L, ref = pkg.lib(), C.byref
    h = C.c_void_p(0x1234)
    good = pkg.rds_soft_opts()
    assert L.sdr_rds_dec_create_soft(None, 0, 4, ref(good)) == INVALID
    assert L.sdr_rds_dec_create_soft(ref(h), 0, 4, None) == INVALID and h.value is None       # *out is cleared
    for nch in (0, -1):
        assert L.sdr_rds_dec_create_soft(ref(h), 0, nch, ref(good)) == INVALID, nch
    for bad in (dict(soft_bits=-1), dict(soft_bits=7), dict(max_burst=-1), dict(max_burst=6), dict(loss_blocks=0),
                dict(loss_blocks=65)):
        assert L.sdr_rds_dec_create_soft(ref(h), 0, 4, ref(pkg.rds_soft_opts(**bad))) == INVALID, bad
        with pytest.raises(ValueError):
            sm.Channel(**bad)
    assert b"soft_bits" in (L.sdr_rds_dec_create_soft(ref(h), 0, 4, ref(pkg.rds_soft_opts(soft_bits=7))), L.sdr_last_error())[1]
    assert h.value is None


def test_calls_refuse(pkg):
    """Every refusal comes before a HIP call, so stand-ins for the handles (zeroed memory: never a tracker, and a
    decoder that was not made by sdr_rds_dec_create_soft) show them without a GPU."""
    L = pkg.lib()
    stand_in = C.create_string_buffer(256)
    row, nb, bits, soft = (C.c_float * 8)(), (C.c_int32 * 1)(), (C.c_uint8 * 256)(), (C.c_uint16 * 256)()
    t, x, n_, b_, s_ = (C.addressof(v) for v in (stand_in, row, nb, bits, soft))
    call = L.sdr_rds_track_bits_soft
    assert call(None, x, 8, 8, n_, b_, 256, s_, 256, None) == INVALID
    assert call(t, None, 8, 8, n_, b_, 256, s_, 256, None) == INVALID
    assert call(t, x, 8, 8, None, b_, 256, s_, 256, None) == INVALID
    assert call(t, x, 8, 8, n_, None, 256, s_, 256, None) == INVALID
    assert call(t, x, 8, 8, n_, b_, 256, None, 256, None) == INVALID and b"soft_dev" in L.sdr_last_error()
    assert call(t, x, 8, 8, n_, b_, 256, s_, 255, None) == INVALID and b"soft_stride" in L.sdr_last_error()
    assert call(t, x, 8, 8, n_, b_, 256, s_ + 1, 256, None) == INVALID          # not a uint16 pointer
    assert call(t, x, 7, 8, n_, b_, 256, s_, 256, None) == INVALID and b"clean_stride" in L.sdr_last_error()
    assert call(t, x, 8, 8, n_, b_, 255, s_, 256, None) == INVALID and b"bits_stride" in L.sdr_last_error()
    assert call(t, x, 8, -1, n_, b_, 256, s_, 256, None) == INVALID
    assert call(t, x, 19713, 19713, n_, b_, 256, s_, 256, None) == INVALID and b"SDR_MAX_BITS" in L.sdr_last_error()
    assert call(t, x + 2, 8, 4, n_, b_, 256, s_, 256, None) == INVALID          # not a float pointer
    call = L.sdr_rds_groups_soft
    assert call(None, n_, b_, 256, s_, 256, None) == INVALID
    assert call(t, None, b_, 256, s_, 256, None) == INVALID
    assert call(t, n_, None, 256, s_, 256, None) == INVALID
    assert call(t, n_, b_, 256, None, 256, None) == INVALID
    assert call(t, n_, b_, 255, s_, 256, None) == INVALID and b"bits_stride" in L.sdr_last_error()
    assert call(t, n_, b_, 256, s_, 255, None) == INVALID and b"soft_stride" in L.sdr_last_error()
    assert call(t, n_, b_, 256, s_ + 1, 256, None) == INVALID
    assert call(t, n_, b_, 256, s_, 256, None) == INVALID and b"sdr_rds_dec_create" in L.sdr_last_error()   # the wrong kind of handle
    assert L.sdr_rds_soft_stats_read(None, s_, None) == INVALID and L.sdr_rds_soft_stats_read(t, None, None) == INVALID
    assert bytes(stand_in) == bytes(256) and nb[0] == 0 and not any(soft)


def test_run_rds_soft_refuses(host, pkg):
    ref = C.byref
    o, good, q = file_opts(), Rds(2, 8), pkg.rds_soft_opts()
    run = host.sdr_multi_run_rds_soft
    assert run(ref(o), None, None, None, None, 0, ref(good), REF, None, ref(q), None) == INVALID      # not on the reference clock
    assert run(ref(o), None, None, None, None, 0, None, TRACK, None, ref(q), None) == INVALID          # no decoder
    for bad in (dict(soft_bits=-1), dict(soft_bits=7), dict(max_burst=6), dict(loss_blocks=0), dict(loss_blocks=65)):
        assert run(ref(o), None, None, None, None, 0, ref(good), TRACK, None, ref(pkg.rds_soft_opts(**bad)), None) == INVALID, bad
    for mode in (1, 2, 3, 4, -1):
        assert run(ref(file_opts(mode=mode)), None, None, None, None, 0, ref(good), TRACK, None, ref(q), None) == INVALID, mode
    for clock in (2, -1):
        assert run(ref(o), None, None, None, None, 0, ref(good), clock, None, ref(q), None) == INVALID, clock
    # what the tracker's entry refuses stays refused with soft == NULL and with it
    for soft in (None, ref(q)):
        assert run(None, None, None, None, None, 0, ref(good), TRACK, None, soft, None) == INVALID
        assert run(ref(o), None, None, None, None, 0, ref(Rds(6, 8)), TRACK, None, soft, None) == INVALID
        assert run(ref(file_opts(nch=0)), None, None, None, None, 0, ref(good), TRACK, None, soft, None) == INVALID
        assert run(ref(o), None, None, None, None, 0, ref(good), TRACK, ref(pkg.rds_track_opts(qshift=16)), soft, None) == INVALID


@pytest.mark.parametrize("args", [
    ["--rds-soft", "6"],                                                     # without --rds-decode
    ["--rds-decode", "--rds-soft", "6"],                                     # without --rds-clock track
    ["--rds-decode", "--rds-clock", "ref", "--rds-soft", "6"],
    ["--rds-decode", "--rds-clock", "track", "--rds-soft", "0"],
    ["--rds-decode", "--rds-clock", "track", "--rds-soft", "7"],
    ["--rds-decode", "--rds-clock", "track", "--rds-soft", "-1"],
    ["--rds-decode", "--rds-clock", "track", "--rds-soft", "six"],
    ["--rds-decode", "--rds-clock", "track", "--rds-soft"],
    ["--rds-decode", "--rds-clock", "track", "--rds-soft", "6", "--mode", "1"],
    ["--rds-decode", "--rds-clock", "track", "--rds-soft", "6", "--scan"],
])
def test_cli_refuses(args, tmp_path):
    assert EXE.exists(), "build with make"
    r = subprocess.run([str(EXE), "2", "--in", "/nonexistent/sdr_multi_rds.u8", "--out", str(tmp_path / "rx"), *args],
                       capture_output=True, text=True, timeout=30)
    assert r.returncode == 1 and r.stderr.startswith("usage: sdr_multi"), r.stderr
    assert "--rds-soft" in r.stderr and not list(tmp_path.iterdir())
