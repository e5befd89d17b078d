"""CPU (no GPU): the band scan's host side -- geometry, the Hann table, and the picker sdr_scan_pick
against the Python restatement of its rule in tests/scan_model.py, on hand-made spectra and on the
f64 model's spectrum of the composite capture (stations at -600, 0 and +500 kHz)."""
from __future__ import annotations

import numpy as np
import pytest

import scan_model as sm


def test_version_and_geometry(pkg):
    assert pkg.lib().sdr_version() == 3
    want = {0: (2400, 30, 73500), 1: (1440, 36, 52920), 2: (2400, 33, 80000), 3: (1152, 33, 38400)}
    for mode, g in want.items():
        assert pkg.scan_geometry(mode) == g
        assert g[0] == pkg.tuner_table(mode).shape[0], "the scan's bins are the tuner's steps"
        assert g[1] == g[2] // g[0]
    for mode in (-1, 4):
        with pytest.raises(pkg.SdrError) as e:
            pkg.scan_geometry(mode)
        assert e.value.code == -1


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_window_bits(pkg, mode):
    N = pkg.scan_geometry(mode)[0]
    w = pkg.scan_window(mode)
    j = np.arange(N, dtype=np.float64)
    want = np.float32(0.5 - 0.5 * np.cos(2 * np.pi * j / N))
    assert w.dtype == np.float32 and w.shape == (N,)
    assert np.array_equal(w.view(np.uint32), want.view(np.uint32))
    assert w[0] == 0.0 and w[N // 2] == 1.0
    # the reference's form of the same window
    assert np.allclose(w, np.sin(np.pi * j / N) ** 2, rtol=0, atol=2.0 ** -24)


def _plateaus(N, at, height=100.0, floor=1.0, half=60):
    """A flat floor with flat-topped stations of 2*half + 1 bins at the given kHz."""
    p = np.full(N, floor, np.float32)
    for k, h in (at.items() if isinstance(at, dict) else ((k, height) for k in at)):
        p[np.arange(k - half, k + half + 1) % N] = h
    return p


def _same(pkg, mode, row, **opts):
    khz, db = pkg.scan_pick(mode, row, **opts)
    wk, wdb = sm.pick(row, **opts)
    assert khz.tolist() == wk, (khz.tolist(), wk)
    assert np.allclose(db, np.array(wdb, np.float32), rtol=1e-6, atol=1e-5, equal_nan=True), (db, wdb)
    assert khz.dtype == np.int32 and db.dtype == np.float32
    return khz.tolist(), db


def test_pick_plateaus(pkg):
    row = _plateaus(2400, {-900: 50.0, -300: 200.0, 0: 100.0, 700: 400.0}, half=20)
    khz, db = _same(pkg, 0, row)
    assert khz == [700, -300, 0, -900]                        # descending channel power
    assert np.all(np.diff(db) < 0) and db[-1] > 10.0
    for mode, N in ((1, 1440), (3, 1152)):
        khz, _ = _same(pkg, mode, _plateaus(N, [-400, 300], half=20))
        assert khz == [-400, 300]                             # equal powers: ascending khz


def test_pick_equal_peaks_lower_khz_wins(pkg):
    # two equal stations 100 kHz apart (within sep = 150): their channel sums are equal bit for bit
    row = _plateaus(2400, [200, 300], half=20)
    khz, _ = _same(pkg, 0, row)
    assert khz == [200]
    # further apart than sep, both are stations, and so are their outer neighbours (21 of the 41
    # station bins in their channel: over the threshold); each tie in ascending khz
    khz, _ = _same(pkg, 0, row, sep_khz=99)
    assert khz == [200, 300, 100, 400]


def test_pick_guard_edge(pkg):
    N = 2400
    khz, _ = _same(pkg, 0, _plateaus(N, [N // 2 - 100], half=0), step_khz=1, half_width_khz=0, sep_khz=400)
    assert khz == [N // 2 - 100]                               # exactly at N/2 - guard: kept
    khz, _ = _same(pkg, 0, _plateaus(N, [N // 2 - 99], half=0), step_khz=1, half_width_khz=0, sep_khz=400)
    assert khz == []                                           # 1 kHz beyond: no candidate there
    khz, _ = _same(pkg, 0, _plateaus(N, [-N // 2 + 100], half=0), step_khz=1, half_width_khz=0, sep_khz=400)
    assert khz == [-N // 2 + 100]


def test_pick_step_and_first(pkg):
    row = _plateaus(2400, [37, -451], half=3)
    khz, _ = _same(pkg, 0, row, step_khz=1, half_width_khz=3, sep_khz=10)
    assert sorted(khz) == [-451, 37]
    row = _plateaus(2400, [-650, 50, 450])
    khz, _ = _same(pkg, 0, row, first_khz=50)
    assert sorted(khz) == [-650, 50, 450]
    khz, _ = _same(pkg, 0, row, first_khz=-1150)      # the same grid, named from its other end
    assert sorted(khz) == [-650, 50, 450]
    khz, _ = _same(pkg, 0, _plateaus(2400, [300]), first_khz=50, sep_khz=0)   # off the grid: its two neighbours tie
    assert khz == [250, 350]


def test_pick_zero_rows(pkg):
    khz, db = _same(pkg, 0, np.zeros(2400, np.float32))
    assert khz == [] and db.size == 0
    row = np.zeros(2400, np.float32)
    row[np.arange(440, 561)] = 3.0                               # one plateau on zeros: F = 0
    khz, db = _same(pkg, 0, row)
    assert khz == [500] and np.isposinf(db[0])


def test_pick_max_smaller_than_found(pkg):
    row = _plateaus(2400, {-900: 50.0, -300: 200.0, 0: 100.0, 700: 400.0}, half=20)
    import ctypes as C
    o = pkg.scan_opts()
    khz, db = np.full(4, 99999, np.int32), np.full(4, -1.0, np.float32)
    n = C.c_int(0)
    rc = pkg.lib().sdr_scan_pick(0, row.ctypes.data_as(C.c_void_p), C.byref(o), khz.ctypes.data_as(C.c_void_p),
                                 db.ctypes.data_as(C.c_void_p), 2, C.byref(n))
    assert rc == 0 and n.value == 4
    assert khz.tolist() == [700, -300, 99999, 99999] and db[2] == -1.0
    rc = pkg.lib().sdr_scan_pick(0, row.ctypes.data_as(C.c_void_p), C.byref(o), None, None, 0, C.byref(n))
    assert rc == 0 and n.value == 4
    k2, d2 = pkg.scan_pick(0, row, max=3)
    assert k2.tolist() == [700, -300, 0] and d2.size == 3


def test_pick_invalid(pkg):
    row = np.ones(2400, np.float32)
    bad = [dict(half_width_khz=-1), dict(half_width_khz=1200), dict(step_khz=0), dict(step_khz=-100),
           dict(sep_khz=-1), dict(guard_khz=-1), dict(guard_khz=1201), dict(thr_db=float("nan")),
           dict(thr_db=float("inf"))]
    for opts in bad:
        with pytest.raises(pkg.SdrError) as e:
            pkg.scan_pick(0, row, **opts)
        assert e.value.code == -1, opts
    with pytest.raises(pkg.SdrError):
        pkg.scan_pick(4, row)
    with pytest.raises(pkg.SdrError):
        pkg.scan_pick(1, row)                                    # 2400 bins are not mode 1's 1440
    with pytest.raises(pkg.SdrError):
        pkg.scan_pick(0, row, bandwidth=3)
    import ctypes as C
    o, n = pkg.scan_opts(), C.c_int(0)
    L = pkg.lib()
    assert L.sdr_scan_pick(0, None, C.byref(o), None, None, 0, C.byref(n)) == -1
    assert L.sdr_scan_pick(0, row.ctypes.data_as(C.c_void_p), None, None, None, 0, C.byref(n)) == -1
    assert L.sdr_scan_pick(0, row.ctypes.data_as(C.c_void_p), C.byref(o), None, None, 0, None) == -1
    assert L.sdr_scan_pick(0, row.ctypes.data_as(C.c_void_p), C.byref(o), None, None, 1, C.byref(n)) == -1
    # the widest legal options still work
    assert pkg.scan_pick(0, row, half_width_khz=1199, guard_khz=1200, step_khz=1, thr_db=0.0)[0].tolist() == [0]


@pytest.mark.parametrize("nblocks", [1, 2])
def test_pick_on_model_spectrum_of_composite(pkg, synth, nblocks):
    """With the default options the composite's stations are exactly {-600, 0, 500}, with room: the
    stations stand tens of dB over the floor, their +-100 kHz neighbours at least 1 dB below them
    (the local-maximum rule decides), everything else far below the 10 dB threshold."""
    comp = sm.composite(synth, 2)[0]
    A, _tol, S = sm.rows_power(pkg, 0, [comp[b][None, :] for b in range(nblocks)])
    psd = (A[0] / S).astype(np.float32)
    khz, db = _same(pkg, 0, psd)
    assert sorted(khz) == [-600, 0, 500]
    assert np.all(db > 30.0)
    # the margins: every candidate's level over the floor (threshold and separation off)
    allk, alldb = pkg.scan_pick(0, psd, thr_db=-1000.0, sep_khz=0)
    level = dict(zip(allk.tolist(), alldb.tolist()))
    assert len(level) == 23
    for k in (-600, 0, 500):
        for nb in (k - 100, k + 100):
            assert level[k] - level[nb] >= 1.0, (k, nb, level[k], level[nb])
    others = [v for k, v in level.items() if all(abs(k - s) > 100 for s in (-600, 0, 500))]
    assert max(others) <= 5.0, max(others)
