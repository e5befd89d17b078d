"""CPU: the reception meter's host side (include/sdr_amd.h: sdr_meter_row, sdr_meter_taps,
sdr_meter_status, the NULL refusals) and the margins of its flags on the model of tests/meter_model.py,
one channel per synthetic kind. No GPU is touched."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import meter_model as mm

IF_FS = {0: 240000, 1: 360000, 2: 240000, 3: 384000}


def test_row_layout(pkg):
    assert C.sizeof(pkg.MeterRow) == 64 and mm.ROW_DTYPE.itemsize == 64
    want = {"fm_sum": 0, "fm_sq": 4, "fm_peak": 8, "pilot_sq": 12, "noise_sq": 16, "rds_sq": 20, "eye_abs": 24,
            "eye_sq": 28, "eye_n": 32, "flags": 36, "l_peak": 40, "r_peak": 44, "l_sq": 48, "r_sq": 56}
    assert [n for n, _ in pkg.MeterRow._fields_] == list(want)
    for name, off in want.items():
        assert getattr(pkg.MeterRow, name).offset == off, name
        assert mm.ROW_DTYPE.fields[name][1] == off, name
    assert pkg.meter_row_dtype() == mm.ROW_DTYPE
    assert pkg.lib().sdr_version() == 3          # the meter is detected by symbol, not by version


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_taps(pkg, mode):
    h = pkg.meter_taps(mode)
    want = pkg.impulse_response_bpf(float(IF_FS[mode]), 75e3, 84e3, 101)
    assert h.dtype == np.float32 and h.shape == (101,)
    assert np.array_equal(h.view(np.uint32), want.view(np.uint32))
    n = C.c_int(0)
    assert pkg.lib().sdr_meter_taps(mode, None, 0, C.byref(n)) == 0 and n.value == 101
    short = np.zeros(100, np.float32)
    assert pkg.lib().sdr_meter_taps(mode, short.ctypes.data_as(C.c_void_p), 100, C.byref(n)) == -1
    assert not short.any()


def _row(**f):
    r = np.zeros((), mm.ROW_DTYPE)
    for k, v in f.items():
        r[k] = v
    return r


def _same(a: float, b: float) -> bool:
    return (math.isnan(a) and math.isnan(b)) or a == b


def _below(v):
    return np.nextafter(np.float32(v), np.float32(0))


# mode 0: n = 7350, n / 5 = 1470, so pilot_sq = 7350 over noise_sq = 1470 is a ratio of exactly 1
HAND_ROWS = [
    ("all zero", _row(), {}, 0),
    ("audio written, silent", _row(flags=1), {}, mm.DEAD_AIR),
    ("silence at the threshold", _row(flags=3, l_peak=64, r_peak=64, l_sq=9, r_sq=9), {}, mm.DEAD_AIR),
    ("one peak above it", _row(flags=1, l_peak=64, r_peak=65), {}, 0),
    ("audio part not written", _row(flags=2, l_peak=0, r_peak=0), {}, 0),
    ("pilot at the threshold", _row(pilot_sq=7350, noise_sq=1470, l_peak=99, r_peak=99), {}, mm.STEREO),
    ("pilot just below", _row(pilot_sq=_below(7350), noise_sq=1470), {}, 0),
    ("rds at the threshold", _row(rds_sq=4 * 7350, noise_sq=1470), {}, mm.RDS),
    ("rds just below", _row(rds_sq=_below(4 * 7350), noise_sq=1470), {}, 0),
    ("offset at the threshold", _row(fm_sum=0.25 * 7350, fm_sq=900.0), {}, mm.OFFTUNE),
    ("negative offset", _row(fm_sum=-0.25 * 7350, fm_sq=900.0), {}, mm.OFFTUNE),
    ("offset just below", _row(fm_sum=_below(0.25 * 7350), fm_sq=900.0), {}, 0),
    ("zero noise under a pilot", _row(pilot_sq=1e-3, noise_sq=0, rds_sq=0), {}, mm.STEREO),
    ("zero noise under both", _row(pilot_sq=2.5, noise_sq=0, rds_sq=1e-30), {}, mm.STEREO | mm.RDS),
    ("zero numerators", _row(pilot_sq=0, rds_sq=0, noise_sq=3.0), {}, 0),
    ("constant eye (zero variance)", _row(eye_abs=10.0, eye_sq=20.0, eye_n=5), {}, 0),
    ("eye_n = 0", _row(eye_abs=10.0, eye_sq=20.0, eye_n=0), {}, 0),
    ("open eye", _row(eye_abs=300.0, eye_sq=1300.0, eye_n=73, rds_sq=1e4, noise_sq=10.0), {}, mm.RDS),
    ("everything", _row(fm_sum=-5300.0, fm_sq=4000.0, fm_peak=1.5, pilot_sq=33.0, noise_sq=0.7, rds_sq=19.0,
                        eye_abs=1234.5, eye_sq=30000.0, eye_n=73, flags=3, l_peak=3, r_peak=64, l_sq=7, r_sq=8), {},
     mm.STEREO | mm.RDS | mm.OFFTUNE | mm.DEAD_AIR),
    ("other thresholds", _row(fm_sum=700.0, pilot_sq=7350, noise_sq=1470, rds_sq=3 * 7350, flags=1, l_peak=100),
     dict(pilot_nr_min=1.5, rds_nr_min=3.0, offtune_min=0.05, silence_peak=100), mm.RDS | mm.OFFTUNE | mm.DEAD_AIR),
    ("NaN readings", _row(fm_sum=np.nan, fm_sq=np.nan, pilot_sq=np.nan, noise_sq=1.0, rds_sq=np.inf), {}, mm.RDS),
]


@pytest.mark.parametrize("what,row,opts,flags", HAND_ROWS, ids=[h[0] for h in HAND_ROWS])
def test_status_equals_python(pkg, what, row, opts, flags):
    got = pkg.meter_status(0, row, **opts)
    want = mm.status(0, row, **opts)
    for k in ("offset", "level_db", "pilot_nr", "rds_nr", "eye_db"):
        assert _same(float(got[k]), want[k]), f"{what}: {k} {got[k]} != {want[k]}"
    assert int(got["flags"]) == want["flags"] == flags, what


def test_status_values_and_modes(pkg):
    """The zero-denominator cases by value, and n of every mode."""
    s = pkg.meter_status(0, _row(pilot_sq=1.0, rds_sq=0.0, noise_sq=0.0, eye_abs=10.0, eye_sq=20.0, eye_n=5))
    assert s["pilot_nr"] == math.inf and s["rds_nr"] == 0.0 and s["eye_db"] == math.inf
    assert s["level_db"] == -math.inf and s["offset"] == 0.0
    s = pkg.meter_status(0, _row())
    assert s["pilot_nr"] == 0.0 and s["eye_db"] == -math.inf and int(s["flags"]) == 0
    for mode, n in mm.BLOCK_IF.items():
        row = _row(fm_sum=float(n), fm_sq=float(10 * n), pilot_sq=float(3 * n), noise_sq=float(n // 5))
        s = pkg.meter_status(mode, row)
        assert s["offset"] == 1.0 and s["level_db"] == 10.0 and s["pilot_nr"] == 3.0, mode
        assert mm.status(mode, row)["pilot_nr"] == 3.0
    rows = np.stack([_row(fm_sum=7350.0), _row()])
    assert pkg.meter_status(0, rows).shape == (2,)
    o = pkg.meter_opts()
    assert (o.pilot_nr_min, o.rds_nr_min, o.offtune_min, o.silence_peak) == (1.0, 4.0, 0.25, 64)
    with pytest.raises(pkg.SdrError):
        pkg.meter_status(0, _row(), no_such_option=1)


def test_null_and_mode_refusals(pkg):
    L = pkg.lib()
    vp = C.c_void_p
    row, o, st = pkg.MeterRow(), pkg.meter_opts(), pkg.MeterState()
    assert L.sdr_meter_create(None, 0, 1, 0) == -1
    assert L.sdr_meter_destroy(None) == -1
    assert L.sdr_meter_reset(None, None) == -1
    assert L.sdr_meter_audio(None, None, None, 0, None) == -1
    assert L.sdr_meter_rds(None, None, None) == -1
    assert L.sdr_meter_read(None, None, None) == -1
    assert L.sdr_meter_rows(None, C.byref(vp())) == -1
    assert L.sdr_meter_status(0, None, C.byref(o), C.byref(st)) == -1
    assert L.sdr_meter_status(0, C.byref(row), None, C.byref(st)) == -1
    assert L.sdr_meter_status(0, C.byref(row), C.byref(o), None) == -1
    assert L.sdr_meter_status(4, C.byref(row), C.byref(o), C.byref(st)) == -1
    assert L.sdr_meter_taps(-1, None, 0, C.byref(C.c_int())) == -1
    h = vp()
    assert L.sdr_meter_create(C.byref(h), 0, 1, 7) == -1 and not h.value      # bad mode: before any device call
    assert L.sdr_meter_create(C.byref(h), 0, 0, 0) == -1 and not h.value      # nch < 1
    L.sdr_meter_opts_default(None)                                            # tolerated, like the scan's


# ---------------------------------------------------------------- margins of the flags on the model
NBLOCKS, CHECK = 10, range(6, 10)


@pytest.fixture(scope="module")
def kind_rows(oracle, synth):
    """rows [kind][block] of the model, mode 0: one channel per synth.KINDS entry, bytes made on the CPU."""
    import torch
    gen = synth.TorchMultiplexBatch(torch, len(synth.KINDS), 0, "cpu", kinds=synth.KINDS, seed=11)
    blocks = np.stack([gen.next_block().numpy().copy() for _ in range(NBLOCKS)])
    return {k: mm.run_rows(oracle, 0, blocks[:, c]) for c, k in enumerate(synth.KINDS)}


def test_flag_margins_on_the_model(kind_rows):
    """STEREO, RDS and OFFTUNE where they must and must not show, each reading a factor of 2 from its
    threshold (pilot_nr 1, rds_nr 4, |offset| 0.25). saturated, dc, weak and rail sit closer to the
    thresholds and are only compared with the model on the GPU."""
    stereo_on, stereo_off = ("normal", "pilot_offset", "carrier_offset"), ("no_pilot", "noise", "silence")
    rds_on, rds_off = ("normal", "pilot_offset", "carrier_offset", "no_pilot"), ("no_rds", "noise", "silence")
    named = set(stereo_on + stereo_off + rds_on + rds_off)
    for kind in sorted(named):
        for b in CHECK:
            s = mm.status(0, kind_rows[kind][b])
            w = f"{kind} block {b}: {s}"
            print(w)
            if kind in stereo_on:
                assert s["pilot_nr"] >= 2 * 1.0 and s["flags"] & mm.STEREO, w
            if kind in stereo_off:
                assert s["pilot_nr"] <= 1.0 / 2 and not s["flags"] & mm.STEREO, w
            if kind in rds_on:
                assert s["rds_nr"] >= 2 * 4.0 and s["flags"] & mm.RDS, w
            if kind in rds_off:
                assert s["rds_nr"] <= 4.0 / 2 and not s["flags"] & mm.RDS, w
            if kind == "carrier_offset":
                assert abs(s["offset"]) >= 2 * 0.25 and s["flags"] & mm.OFFTUNE, w
            else:
                assert abs(s["offset"]) <= 0.25 / 2 and not s["flags"] & mm.OFFTUNE, w


def test_silence_reads_exactly_zero(kind_rows):
    for b in range(NBLOCKS):
        row = kind_rows["silence"][b]
        for name in mm.ROW_DTYPE.names:
            if name not in ("flags", "eye_n"):
                assert row[name] == 0 and not np.signbit(np.float64(row[name])), f"{name} block {b}"
        assert row["flags"] == 3 and row["eye_n"] == 73
        assert mm.status(0, row)["flags"] == mm.DEAD_AIR


def test_tree_sum_order():
    """The summation order itself, on values whose sum depends on it."""
    rs = np.random.Generator(np.random.PCG64(5))
    v = (rs.standard_normal(7350) * 10.0 ** rs.uniform(-6, 6, 7350)).astype(np.float32)
    P = [np.float32(0)] * 256
    for i, x in enumerate(v):
        P[i % 256] = np.float32(P[i % 256] + x)
    w = 128
    while w:
        for p in range(w):
            P[p] = np.float32(P[p] + P[p + w])
        w //= 2
    assert mm.tree_sum(v).view(np.uint32) == P[0].view(np.uint32)
    assert mm.tree_sum(np.zeros(0, np.float32)) == 0 and mm.tree_sum(v[:73], 64).dtype == np.float32
