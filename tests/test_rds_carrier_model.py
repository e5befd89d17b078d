"""CPU: the model of the RDS carrier-phase derotator (tests/rds_carrier_model.py, the definition that
include/sdr_amd.h states for sdr_rds_carrier_*) against its own rules: the result does not depend on the cut,
the sums keep their bounds, the two CORDICs are as accurate as their iteration count allows, a turned stream
comes back on one axis without a flip, and the tracker reads the rows as the integers they are."""
from __future__ import annotations

import math

import numpy as np
import pytest

import rds_carrier_model as cm
import rds_track_model as tm

W = cm.W
OPTIONS = [dict(), dict(qshift=0), dict(qshift=15), dict(avg_shift=0), dict(avg_shift=6), dict(qshift=7, avg_shift=1)]
CUT_SIZES = (0, 1, 2047, 2048, 2049, 2836, 19712)


def _cut(x, sizes):
    at = 0
    for n in sizes:
        yield x[0][at:at + n], x[1][at:at + n]
        at += n
    assert at == len(x[0])


@pytest.mark.parametrize("opts", OPTIONS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "defaults")
def test_the_cut_does_not_matter(opts):
    sizes = (2836, 1, 0, 2047, 19712, 2049, 2048, 1, 2836, 2048, 2047)
    assert set(sizes) == set(CUT_SIZES)
    total = sum(sizes)
    q = opts.get("qshift", cm.QSHIFT)
    x = cm.off_grid(5, total, 37.0, qshift=q)
    want, one = cm.derotate(_cut(x, (19712, total - 19712)), **opts)
    got, ch = cm.derotate(_cut(x, sizes), **opts)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and ch.state() == one.state()
    rows, blocks = cm.derotate(_cut(x, [2836] * (total // 2836) + [total % 2836]), **opts)
    assert np.array_equal(rows.view(np.uint32), want.view(np.uint32)) and blocks.state() == one.state()
    assert one.windows == total // W and one.wcnt == total % W and one.resets == 0
    # the stream is worth the test: a phase was estimated, and the specials reached the clamp
    assert one.phi != 0 and (one.c, one.s) != (cm.ONE, 0)
    assert np.abs(cm.quantise(x[0], q)).max() == cm.QMAX


def test_full_scale_rows_keep_the_int64_bounds():
    """Both rows at the clamp for whole windows: a window's sums reach their bound W * 2^31 (to within the
    clamp's 32767 < 2^15) and S, with avg_shift 0 a copy of them, too; nothing is near 2^63."""
    n = 3 * W
    big = np.full(n, 3e38, np.float32)
    for si, sq in ((1, 1), (1, -1), (-1, -1)):
        ch = cm.Channel(avg_shift=0)
        ch.call(si * big, sq * big)
        assert (ch.sr, ch.si, ch.st) == (0, si * sq * 2 * W * cm.QMAX ** 2, 2 * W * cm.QMAX ** 2)
        assert ch.st <= cm.P_MAX < 1 << 63 and ch.st > cm.P_MAX - (1 << 28)
        assert abs(abs(ch.phase_deg()) - 45.0) < 1e-3 and ch.windows == 3
    ch = cm.Channel(avg_shift=6)
    ch.call(big, np.zeros(n, np.float32))
    assert ch.si == 0 and 0 < ch.sr == ch.st < W * cm.QMAX ** 2 and abs(ch.phi) < 300 and (ch.c, ch.s) == (cm.ONE, 0)
    # the rotation at the clamp: |qi c + qq s| is largest at 45 degrees and still below 2^31 (the model asserts it)
    ch = cm.Channel(avg_shift=0)
    y = ch.call(big, big)
    assert ch.y[:W].tolist() == [cm.QMAX] * W and ch.y[W:].tolist() == [cm.QMAX] * (2 * W)   # sqrt(2) * 32767, clamped
    assert float(y[0]) == cm.QMAX / 1024.0


# What N iterations can give. Vectoring: the angle left after the last step is at most atan(2^-(N-1)); every step
# floors two shifted terms, an error below one unit in x and in y, which later steps turn and scale by at most the
# CORDIC's gain: N * sqrt(2) * 1.6468 units in all, seen from a vector of at least 2^28 units; the table's entries
# are rounded, half a unit of angle each, and the halved result once more.
_TRUNC = cm.N_CORDIC * math.sqrt(2) * 1.6468
ANGLE_BOUND = (math.atan(2.0 ** -(cm.N_CORDIC - 1)) + _TRUNC / 2 ** 28) * 2 ** 32 / (2 * math.pi) + cm.N_CORDIC / 2 + 1
# Rotation: the same residual and table error in the angle, times 2^14; the same truncation, in units of 2^-29,
# shifted down by 15; half a unit for the final rounding.
VECTOR_BOUND = 0.5 + cm.ONE * (math.atan(2.0 ** -(cm.N_CORDIC - 1)) + cm.N_CORDIC / 2 * 2 * math.pi / 2 ** 32) + _TRUNC / 2 ** 15


def test_cordic_angle_against_atan2():
    assert ANGLE_BOUND < 300                                  # 2.6e-5 degrees
    rs = np.random.Generator(np.random.PCG64(1))
    pairs = [(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1), (5, -3), (1 << 42, 1), (-(1 << 42), -1),
             (-(1 << 42), 1), (1 << 29, 1 << 29), (-(1 << 29), 1 << 29), (3, 1 << 41)]
    pairs += [(int(a), int(b)) for a, b in rs.integers(-(1 << 42), 1 << 42, (4000, 2))]
    pairs += [(int(a), int(b)) for a, b in rs.integers(-2000, 2000, (1000, 2)) if a or b]
    worst = 0.0
    for sr, si in pairs:
        x, y = cm.normalise(sr, si)
        assert 1 << 28 <= max(abs(x), abs(y)) <= 1 << 29
        got = cm.cordic_angle(x, y)
        want = math.atan2(y, x) / (2 * math.pi) * 2 ** 32      # of the shifted pair: the shift's own floor is the input's
        err = abs(cm.wrap32(got - round(want)))
        worst = max(worst, err)
        assert err <= ANGLE_BOUND, (sr, si, got, want)
        if max(abs(sr), abs(si)) < 1 << 28:                     # a left shift is exact: against the pair itself
            assert abs(cm.wrap32(got - round(math.atan2(si, sr) / (2 * math.pi) * 2 ** 32))) <= ANGLE_BOUND
    print(f"vectoring CORDIC: worst error {worst:.0f} of 2^32 a turn, bound {ANGLE_BOUND:.0f}")


def test_cordic_vector_against_cos_sin():
    assert VECTOR_BOUND < 0.51
    rs = np.random.Generator(np.random.PCG64(2))
    angles = [0, 1, -1, 1 << 30, -(1 << 30), (1 << 30) + 1, -(1 << 30) - 1, (1 << 31) - 1, -(1 << 31), 1 << 29, -(1 << 29),
              3 << 29, -(3 << 29)] + [int(v) for v in rs.integers(-(1 << 31), 1 << 31, 5000)]
    worst = 0.0
    for phi in angles:
        c, s = cm.cordic_vector(phi)
        a = phi * 2 * math.pi / 2 ** 32
        err = max(abs(c - cm.ONE * math.cos(a)), abs(s - cm.ONE * math.sin(a)))
        worst = max(worst, err)
        assert err <= VECTOR_BOUND, (phi, c, s)
    assert cm.cordic_vector(0) == (cm.ONE, 0) and cm.cordic_vector(1 << 30) == (0, cm.ONE)
    assert cm.cordic_vector(-(1 << 31)) == (-cm.ONE, 0) and cm.cordic_vector(-(1 << 30)) == (0, -cm.ONE)
    print(f"rotation CORDIC: worst error {worst:.4f} of 2^-14, bound {VECTOR_BOUND:.4f}")


@pytest.mark.parametrize("deg", [30.0, 120.0, -60.0, -150.0, 45.0, -44.5, 89.0, 91.0, 179.0, 0.0])
def test_a_turned_stream_comes_back(deg):
    """Chips of +-300 turned by deg: after the first windows the phase in use is deg modulo 180 and the output is
    the chips again, of one constant sign, at nearly their full level (the noise of both rows is in it)."""
    n = 9 * W                                                 # one call, below MAX_N
    xi, xq, lvl = cm.rotated(21, n, deg)
    y, ch = cm.derotate([(xi, xq)])
    err = (ch.phase_deg() - deg + 90) % 180 - 90
    assert abs(err) < 1.5, (deg, ch.phase_deg())
    assert ch.coherence() > 0.75                              # 300^2 against 300^2 + 2 * 120^2 / 3 of uniform noise
    got = ch.y[4 * W:].astype(np.float64)
    gain = float(np.mean(got * lvl[4 * W:])) / 300.0 ** 2
    assert abs(gain) > 0.98, gain
    per_window = np.sign(np.sum((ch.y * lvl)[W:].reshape(-1, W), axis=1))   # window 0 is not rotated yet
    assert np.all(per_window == per_window[0])
    # the first window is the in-phase row itself
    assert np.array_equal(ch.y[:W], cm.quantise(xi[:W]))


@pytest.mark.parametrize("turn", [360.0, -360.0])
def test_a_slow_ramp_keeps_its_branch(turn):
    """The carrier phase walks a whole turn in 160 windows, through +-90 degrees, where half the angle changes
    branch, and through +-180, where the int32 angle wraps: the phase in use follows without a jump and the
    output never changes sign."""
    nwin = 160
    n = nwin * W
    deg = 60.0 + turn * np.arange(n) / n
    xi, xq, lvl = cm.rotated(22, n, deg)
    ch = cm.Channel()
    phis, signs = [], []
    for w in range(nwin):
        ch.call(xi[w * W:(w + 1) * W], xq[w * W:(w + 1) * W])
        phis.append(ch.phase_deg())
        signs.append(np.sign(np.sum(ch.y * lvl[w * W:(w + 1) * W])))
    steps = (np.diff(phis) + 180) % 360 - 180
    assert np.abs(steps[4:]).max() < 10.0, np.abs(steps).max()          # 2.25 degrees a window, no half turn
    assert len(set(signs[4:])) == 1 and signs[4] != 0
    total = float(np.sum(steps))
    assert abs(total - turn) < 40.0, total                               # the whole turn, less the smoothing's lag
    assert min(phis) < -150 and max(phis) > 150                          # it did cross the wrap


def test_zeros_keep_the_phase():
    xi, xq, _ = cm.rotated(23, 6 * W, 70.0)
    for k in (0, 3):
        ch = cm.Channel(avg_shift=k)
        ch.call(xi, xq)
        before = (ch.phi, ch.c, ch.s)
        assert abs(ch.phase_deg() - 70.0) < 1.5
        z = np.zeros(W, np.float32)
        for _ in range(80):                                    # with avg_shift 3, S decays: its angle stays while
            ch.call(z, z)                                      # S is large enough to have one
            assert abs(ch.phase_deg() - 70.0) < 1.5 or max(abs(ch.sr), abs(ch.si)) < 1 << 10
            if k == 0:
                assert (ch.sr, ch.si, ch.st) == (0, 0, 0) and (ch.phi, ch.c, ch.s) == before
        assert ch.windows == 86
    fresh = cm.Channel()
    y = fresh.call(np.zeros(3 * W, np.float32), np.zeros(3 * W, np.float32))
    assert not y.any() and (fresh.phi, fresh.c, fresh.s) == (0, cm.ONE, 0) and fresh.windows == 3


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("row", [0, 1])
def test_a_non_finite_sample_resets_the_channel(bad, row):
    xi, xq, _ = cm.rotated(24, 5 * W + 100, -30.0)
    ch = cm.Channel()
    ch.call(xi[:3 * W + 7], xq[:3 * W + 7])
    assert ch.phi != 0 and ch.wcnt == 7
    rows = [xi[3 * W + 7:4 * W].copy(), xq[3 * W + 7:4 * W].copy()]
    rows[row][-1] = bad
    y = ch.call(*rows)
    assert len(y) == W - 7 and np.isnan(y).all()
    fresh = cm.Channel()
    assert ch.state()[:-3] == fresh.state()[:-3] and ch.resets == 1 and ch.windows == 3
    # the stream starts again: the next rows are those of a new channel
    a = ch.call(xi[4 * W:], xq[4 * W:])
    b = fresh.call(xi[4 * W:], xq[4 * W:])
    assert np.array_equal(a, b) and ch.wcnt == 100
    # and the tracker behind it reports the call as poisoned
    assert tm.Channel().call(y)[0] == tm.NBITS_POISONED
    with pytest.raises(ValueError):
        ch.call(np.zeros(cm.MAX_N + 1, np.float32), np.zeros(cm.MAX_N + 1, np.float32))


@pytest.mark.parametrize("qshift", [0, 10, 15])
def test_the_tracker_reads_the_integers_back(qshift):
    n = 4 * W
    xi, xq = cm.off_grid(25, n, -44.5, qshift=qshift, gain=120.0)
    ch = cm.Channel(qshift=qshift)
    y = ch.call(xi, xq)
    assert y.dtype == np.float32 and np.array_equal(tm.quantise(y, qshift), ch.y)
    assert np.abs(ch.y).max() == cm.QMAX and len(np.unique(ch.y)) > 500
