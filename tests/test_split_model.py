"""CPU: the wideband splitter's host side (sdr_split_geometry, sdr_split_taps, the refusals that need no
device) and the conventions of the model in tests/split_model.py that the GPU tests compare against."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import split_model as spm

WS = (4, 8, 10)
E_INVALID = -1                      # SDR_E_INVALID (include/sdr_amd.h)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("W", WS)
def test_geometry(pkg, mode, W):
    N, block_iq = spm.GEOM[mode]
    assert pkg.split_geometry(mode, W) == (2 * W - 1, 16 * W, W * block_iq, N // 2, spm.SHIFT_DEFAULT[W])
    assert pkg.scan_geometry(mode)[0] == N and pkg.scan_geometry(mode)[2] == block_iq
    assert block_iq % 2 == 0          # the parity of t is the parity of the index in the block


@pytest.mark.parametrize("W", [0, 1, 2, 5, 6, 9, 12, 16, -8])
def test_refused_width(pkg, W):
    L = pkg.lib()
    n = C.c_int(0)
    assert L.sdr_split_geometry(0, W, None, None, None, None, None) == E_INVALID
    assert L.sdr_split_taps(W, None, 0, C.byref(n)) == E_INVALID
    with pytest.raises(pkg.SdrError):
        pkg.split_geometry(0, W)


@pytest.mark.parametrize("W", WS)
def test_taps(pkg, W):
    g = pkg.split_taps(W)
    T, R = 16 * W, 2 * W - 1
    assert g.shape == (R, T, 2) and g.dtype == np.int16
    re, im = spm.taps_f64(W)
    assert np.abs(g[..., 0] - re).max() <= 0.5 + 1e-6 and np.abs(g[..., 1] - im).max() <= 0.5 + 1e-6
    gi = g.astype(np.int64)
    assert np.all(gi[W - 1, :, 1] == 0)                                      # row W - 1 (k = 0) is real
    assert np.array_equal(gi[:, ::-1, 0], gi[..., 0]) and np.array_equal(gi[:, ::-1, 1], -gi[..., 1])
    assert np.array_equal(gi[::-1, :, 0], gi[..., 0]) and np.array_equal(gi[::-1, :, 1], -gi[..., 1])
    assert np.abs(gi).max() <= 8191
    dc = gi[W - 1, :, 0].sum() * 2.0 ** -spm.SHIFT_DEFAULT[W]
    assert 1.0 <= dc <= 2.01
    # the model's own table agrees entry for entry
    assert np.array_equal(g, spm.taps(W))


def test_taps_room(pkg):
    L = pkg.lib()
    n = C.c_int(0)
    g = np.zeros((7, 64, 2), np.int16)
    assert L.sdr_split_taps(4, g.ctypes.data_as(C.c_void_p), 7 * 64 - 1, C.byref(n)) == E_INVALID
    assert L.sdr_split_taps(4, None, 0, C.byref(n)) == pkg.SDR_OK and n.value == 7 * 64
    assert L.sdr_split_taps(4, g.ctypes.data_as(C.c_void_p), 7 * 64, None) == E_INVALID


def test_refusals_without_device(pkg):
    L = pkg.lib()
    h = C.c_void_p()
    E = E_INVALID
    assert L.sdr_split_geometry(4, 8, None, None, None, None, None) == E
    assert L.sdr_split_geometry(-1, 8, None, None, None, None, None) == E
    assert L.sdr_split_create(None, 0, 0, 8, 1, 0) == E
    assert L.sdr_split_create(C.byref(h), 0, 4, 8, 1, 0) == E and not h.value
    assert L.sdr_split_create(C.byref(h), 0, 0, 5, 1, 0) == E and not h.value
    assert L.sdr_split_create(C.byref(h), 0, 0, 8, 0, 0) == E and not h.value
    assert L.sdr_split_create(C.byref(h), 0, 0, 8, 1, 25) == E and not h.value
    assert L.sdr_split_destroy(None) == E
    assert L.sdr_split_reset(None, None) == E
    assert L.sdr_split_block(None, None, 0, None, 0, None) == E
    assert L.sdr_split_clips(None, None, None) == E
    assert b"split" in L.sdr_last_error()


@pytest.mark.parametrize("k,delta", [(0, 37), (1, -250), (-1, 250), (2, 0), (7, 599), (-7, -600)])
def test_model_convention(pkg, k, delta):
    """Mode 0, W = 8: a tone at F = k N / 2 + delta kHz of the wide capture is the station khz = +delta of
    row k + W - 1: the Hann periodogram of the model's row peaks at bin delta mod N. (The model's taps are
    the library's, entry for entry, so the convention holds for both.)"""
    W, mode = 8, 0
    N, block_iq = spm.GEOM[mode]
    assert np.array_equal(spm.taps(W), pkg.split_taps(W)) and pkg.split_geometry(mode, W)[3] == N // 2
    F = k * N // 2 + delta
    n = np.arange(W * block_iq, dtype=np.int64)
    ph = 2.0 * np.pi * np.mod(F * n, W * N).astype(np.float64) / (W * N)
    wide = np.empty(2 * W * block_iq, np.int8)
    wide[0::2] = np.round(100.0 * np.cos(ph)).astype(np.int8)
    wide[1::2] = np.round(100.0 * np.sin(ph)).astype(np.int8)
    m = spm.SplitModel(mode, W)
    row = m.block(wide)[k + W - 1].astype(np.float64) - 128.0
    z = (row[0::2] + 1j * row[1::2])[N:2 * N]                      # one segment past the start-up
    p = np.abs(np.fft.fft(z * np.hanning(N + 1)[:N])) ** 2
    assert int(np.argmax(p)) == delta % N


def test_wide_pick_rule(pkg):
    """The grid is absolute, the guard is N / 4, and the N / 4 tie goes to the earlier row."""
    W, mode = 4, 1                                                 # N / 2 = 720 is no multiple of 100
    N = spm.GEOM[mode][0]
    assert pkg.split_geometry(mode, W)[:4] == (7, 64, W * spm.GEOM[mode][1], 720)
    calls = []

    def pick(row, **o):
        calls.append(o)
        return list(row), [0.0] * len(row)

    rows = [[] for _ in range(2 * (2 * W - 1))]
    rows[3] = [360, -100]              # k = 0: absolute 360 and -100
    rows[4] = [-360, 80]               # k = 1: absolute 360 (the tie, dropped) and 800
    rows[7 + 4] = [-360]               # the other stream keeps its own
    got = spm.wide_pick(mode, W, rows, pick, first_khz=0, step_khz=100)
    assert got == [(3, 360), (3, -100), (4, 80), (11, -360)]
    assert all(o["guard_khz"] == N // 4 and o["step_khz"] == 100 for o in calls)
    assert [o["first_khz"] for o in calls[:7]] == [(-(r - 3) * 720) % 100 for r in range(7)]
