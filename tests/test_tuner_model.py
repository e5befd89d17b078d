"""CPU: the shared-capture tuner's rotator table, the CPU model the GPU tests compare against
(tests/tuner_model.py), and the tuner entry points' argument checks that need no GPU.

The model test is a condition on the inputs, not on the kernel: the three stations of the composite
capture must come out of the model the way each does alone, or the GPU tests would compare two
equally wrong things."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import tuner_model as tm
from conftest import ROOT, channel_input

RF_FS = {0: 2400000, 1: 1440000, 2: 2400000, 3: 1152000}


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_table_is_the_correctly_rounded_rotator(pkg, mode):
    import mpmath
    N = RF_FS[mode] // 1000
    t = pkg.tuner_table(mode)
    assert t.shape == (N, 2) and t.dtype == np.float32 and N % 4 == 0
    mpmath.mp.dps = 50
    # cospi / sinpi take the argument in half turns, so the exact zeros and ones stay exact
    ref = np.array([[float(mpmath.cospi(mpmath.mpf(2 * i) / N)), float(mpmath.sinpi(mpmath.mpf(2 * i) / N))]
                    for i in range(N)], np.float64)
    # the 50-digit value rounded to f64 and then to f32 equals the value rounded to f32 unless it
    # lies within 2^-53 relative of an f32 tie; no entry of these tables does (checked: the f64 is
    # then exactly a tie, i.e. its low 29 mantissa bits are 1 followed by zeros)
    bits = ref.view(np.uint64) & np.uint64((1 << 29) - 1)
    assert not np.any((bits == np.uint64(1 << 28)) & (ref != 0.0))
    want = ref.astype(np.float32)
    assert np.array_equal(t.view(np.uint32), want.view(np.uint32))
    assert tuple(t[0]) == (1.0, 0.0) and tuple(t[N // 4]) == (0.0, 1.0)
    assert np.array_equal(t.view(np.uint32)[0], np.array([0x3F800000, 0], np.uint32))
    # odd / even symmetry
    assert np.array_equal(t[1:, 0], t[1:, 0][::-1]) and np.array_equal(t[1:, 1], -t[1:, 1][::-1])


def test_table_refuses_bad_arguments(pkg):
    lib = pkg.lib()
    n = C.c_int(0)
    buf = np.zeros((2400, 2), np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.sdr_tuner_table(4, None, 0, C.byref(n)) == -1
    assert lib.sdr_tuner_table(-1, None, 0, C.byref(n)) == -1
    assert lib.sdr_tuner_table(0, p, 2400, None) == -1
    assert lib.sdr_tuner_table(0, p, 2399, C.byref(n)) == -1
    assert lib.sdr_tuner_table(0, None, 0, C.byref(n)) == 0 and n.value == 2400
    assert lib.sdr_tuner_table(1, p, 2400, C.byref(n)) == 0 and n.value == 1440
    with pytest.raises(pkg.SdrError):
        pkg.tuner_table(7)


def test_entry_points_refuse_null_without_a_gpu(pkg):
    lib = pkg.lib()
    assert lib.sdr_version() >= 2
    assert lib.sdr_frontend_tuned(None, None, 0, None) == -1
    assert lib.sdr_tuner_set(None, 0, None, None, None) == -1
    n = C.c_int(5)
    assert lib.sdr_tuner_get(None, C.byref(n)) == -1
    host = C.CDLL(str(ROOT / "real-time-sdr_amd" / "libsdr_host.so"))
    host.sdr_multi_run_tuned.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    assert host.sdr_multi_run_tuned(None, None, None) == -1


def test_model_separates_the_composite_stations(pkg, oracle, synth):
    """10 blocks of mode 0 (the issue's figures on this input: no clipping, identity equal,
    correlation 0.999998, all 12 bit rows equal)."""
    nb = tm.COMPOSITE_BLOCKS
    comp, clipped = tm.composite(synth, nb)
    assert clipped == 0
    # khz = 0 on an identity src is the untuned front end, bit for bit
    ident = tm.run_tuned(pkg, oracle, 0, comp[:, None, :], [0], [0])[0]["fm"]
    ch = oracle.Channel(0, True)
    for b in range(nb):
        assert np.array_equal(ident[b].view(np.uint32), ch.frontend(comp[b]).view(np.uint32)), f"block {b}"
    model = tm.composite_model(pkg, oracle, synth)
    for c in range(3):
        alone = oracle.run_channel(channel_input(synth, c, nb), 0, True)
        a = np.concatenate(alone["mono"][2:nb]).astype(np.float64)
        m = np.concatenate(model[c]["mono"][2:nb]).astype(np.float64)
        corr = float(np.corrcoef(a, m)[0, 1])
        print(f"station {c} ({tm.COMPOSITE_KHZ[c]} kHz): mono correlation {corr:.6f}")
        assert corr >= 0.999
        for b in range(6, nb):
            assert alone["bits"][b] is not None and model[c]["bits"][b] is not None, f"station {c} block {b}"
            assert np.array_equal(alone["bits"][b], model[c]["bits"][b]), f"station {c} block {b} bits"
