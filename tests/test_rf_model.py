"""CPU: the RF meter's host arithmetic (sdr_meter_rf_status, include/sdr_amd.h) against tests/rf_model.py, and what
the readings mean, on the model alone: a carrier in noise reads its true in-channel C/N, noise alone a ripple of
1, a carrier alone a ripple of 0."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import rf_model as rm
from conftest import channel_input

BLOCK_IQ = 73500          # mode 0


def _same(a: float, b: float) -> bool:
    return (math.isnan(a) and math.isnan(b)) or a == b


def _assert_status(pkg, row, what, **opts):
    got = pkg.meter_rf_status(0, row, **opts)
    want = rm.status(row, **opts) if opts else rm.status(row)
    for k in ("level_dbfs", "ripple", "cnr_db", "fade_db", "crest_db"):
        assert _same(float(got[k]), want[k]), f"{what}: {k} {float(got[k])!r} != {want[k]!r}"
    assert int(got["flags"]) == want["flags"], what
    return want


def _row(**f):
    r = np.zeros((), rm.ROW_DTYPE)
    for k, v in f.items():
        r[k] = v
    return r


def test_row_layout(pkg):
    assert C.sizeof(pkg.MeterRfRow) == 32 and pkg.meter_rf_row_dtype().itemsize == 32
    for name in rm.ROW_DTYPE.names:
        assert getattr(pkg.MeterRfRow, name).offset == rm.ROW_DTYPE.fields[name][1], name
    assert pkg.lib().sdr_version() == 3           # detected by symbol, not by version
    o = pkg.meter_rf_opts()
    assert np.float32(o.ripple_max).view(np.uint32) == (np.float32(21.0) / np.float32(121.0)).view(np.uint32)
    with pytest.raises(pkg.SdrError):
        pkg.meter_rf_status(0, _row(), no_such_option=1)


@pytest.fixture(scope="module")
def synth_rows(oracle, synth):
    """The model's rows of two synthetic channels, two blocks each."""
    out = {}
    for c in (0, 1):
        ch = rm.EnvChannel(oracle, 0)
        out[c] = [rm.rf_row(ch.block(iq)) for iq in channel_input(synth, c, 2)]
    return out


def test_status_equals_the_model_on_synthetic_channels(pkg, synth_rows):
    for c, rows in synth_rows.items():
        for b, row in enumerate(rows):
            st = _assert_status(pkg, row, f"ch {c} block {b}")
            assert row["n"] == 7350 and row["flags"] == rm.ROW_RF
            assert math.isfinite(st["level_dbfs"]) and st["level_dbfs"] < 0.0
            _assert_status(pkg, row, f"ch {c} block {b}, a tight threshold", ripple_max=1e-9)
        long_row = rm.run_long(rows)
        assert long_row["n"] == 2 * 7350
        _assert_status(pkg, long_row, f"ch {c}, the run-long row")
    assert pkg.meter_rf_status(0, np.stack(synth_rows[0])).shape == (2,)


def test_status_edge_rows(pkg):
    # an all-zero written row: no level, no ripple, WEAK
    st = _assert_status(pkg, _row(n=7350, flags=rm.ROW_RF), "zero row")
    assert st["level_dbfs"] == -math.inf and st["ripple"] == 0.0 and st["cnr_db"] == -math.inf
    assert st["fade_db"] == 0.0 and st["crest_db"] == 0.0 and st["flags"] == rm.WEAK
    # an unwritten row (all zero, n = 0): the same readings, no WEAK
    st = _assert_status(pkg, _row(), "unwritten row")
    assert st["level_dbfs"] == -math.inf and st["cnr_db"] == -math.inf and st["flags"] == 0
    # 2 m1^2 < m2 (burstier than Gaussian noise): no carrier found
    st = _assert_status(pkg, _row(env_sum=100.0, env_sq=300.0, env_min=0.0, env_max=9.0, n=100, flags=rm.ROW_RF), "2 m1^2 < m2")
    assert st["cnr_db"] == -math.inf and st["ripple"] == 2.0 and st["fade_db"] == -math.inf and st["flags"] == rm.WEAK
    assert _same(st["crest_db"], 10.0 * math.log10(9.0))
    # N <= 0 (m2 = m1^2: a constant envelope): no noise found
    st = _assert_status(pkg, _row(env_sum=25.0, env_sq=6.25, env_min=0.25, env_max=0.25, n=100, flags=rm.ROW_RF), "N = 0")
    assert st["cnr_db"] == math.inf and st["ripple"] == 0.0 and st["fade_db"] == 0.0 and st["flags"] == 0
    assert _same(st["level_dbfs"], 10.0 * math.log10(0.25))
    # the threshold is strict: ripple == ripple_max is not WEAK (S = 10 N: M2 = 11, M4 - M2^2 = 21)
    at = _row(env_sum=11.0, env_sq=142.0, env_min=1.0, env_max=30.0, n=1, flags=rm.ROW_RF)
    st = _assert_status(pkg, at, "rho = 10")
    assert abs(st["cnr_db"] - 10.0) < 1e-9 and st["ripple"] == 21.0 / 121.0
    assert st["flags"] == (rm.WEAK if 21.0 / 121.0 > rm.RIPPLE_MAX else 0)


# ---------------------------------------------------------------- what the readings mean (the model alone)
AMP, SIGMA = 0.3, 0.2


@pytest.fixture(scope="module")
def meaning(oracle):
    """Three mode-0 blocks each of: the carrier in noise, the noise alone, the carrier alone (fixed seeds), through
    one EnvChannel each (so blocks 1 and 2 start from real FIR states)."""
    out = {}
    for name, amp, sigma, seed in (("both", AMP, SIGMA, 101), ("noise", 0.0, SIGMA, 102), ("carrier", AMP, 0.0, 103)):
        ch = rm.EnvChannel(oracle, 0)
        u8 = rm.carrier_noise_u8(3 * BLOCK_IQ, amp, sigma, seed).reshape(3, 2 * BLOCK_IQ)
        out[name] = [rm.status(rm.rf_row(ch.block(b))) for b in u8]
    out["true"] = rm.true_cnr_db(ch.h, AMP, SIGMA)
    return out


def test_carrier_in_noise_reads_its_cnr(meaning):
    """A carrier of amplitude 0.3 at +20 kHz in noise of sigma 0.2 per component: the true in-channel C/N from A^2,
    2 sigma^2 + 2 / (12 128^2) and the real taps' sum h^2 and gain; every block's cnr_db within 0.5 dB of it."""
    true = meaning["true"]
    print("true C/N %.3f dB; estimates %s" % (true, ["%.3f" % s["cnr_db"] for s in meaning["both"]]))
    assert 10.0 < true < 13.5, true
    for b, st in enumerate(meaning["both"]):
        assert abs(st["cnr_db"] - true) < 0.5, (b, st["cnr_db"], true)
        assert abs(st["level_dbfs"] - 10.0 * math.log10(AMP * AMP * (1.0 + 10.0 ** (-true / 10.0)))) < 0.3, (b, st)
        assert st["flags"] == 0                      # above the FM threshold


def test_noise_alone_has_ripple_one(meaning):
    print("noise ripple %s" % ["%.4f" % s["ripple"] for s in meaning["noise"]])
    for b, st in enumerate(meaning["noise"]):
        assert 0.9 <= st["ripple"] <= 1.1, (b, st["ripple"])
        assert st["flags"] == rm.WEAK


def test_carrier_alone_has_no_ripple(meaning):
    print("carrier ripple %s" % ["%.3g" % s["ripple"] for s in meaning["carrier"]])
    for b, st in enumerate(meaning["carrier"]):     # (block 0 holds the FIR's start-up from the zero state: 7.6e-4)
        assert st["ripple"] < 1e-3, (b, st["ripple"])
        assert abs(st["level_dbfs"] - 10.0 * math.log10(AMP * AMP)) < 0.1 and st["flags"] == 0
