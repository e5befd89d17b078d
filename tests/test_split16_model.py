"""CPU: the 16-bit splitter's definition as tests/split16_model.py states it (include/sdr_amd.h, sdr_split16_*):
the bounds of the sums, the two identities that tie it to the s8 splitter's model, independence of how a
capture is cut, the gain rule's two properties, and the library's sdr_split16_shift_for against the model's."""
from __future__ import annotations

import numpy as np
import pytest

import split16_model as s16
import split_model as spm

WS = (4, 8, 10)
MODE = 3                                                            # the smallest block (38400 outputs)


@pytest.mark.parametrize("W", WS)
def test_bounds_and_sums_past_int32(W):
    col, top = s16.bounds(W)
    assert top == {4: 2457993216, 8: 4876533760, 10: 6089736192}[W]
    # a window carrying the signs of the worst column at full scale does pass 2^31 (and the flip keeps |acc|)
    M = spm.tap_matrix(W)
    c = int(np.abs(M).sum(axis=0).argmax())
    m = s16.Split16Model(MODE, W)
    T, t = 16 * W, 40
    x = np.zeros(2 * W * 64, np.int16)
    x[2 * (W * t - T + 1):2 * (W * t + 1)] = np.where(M[:, c] < 0, -32768, 32767)
    acc = m.flipped(x, 64)
    neg = int((M[:, c] < 0).sum())
    want = 32767 * col + int(-M[M[:, c] < 0, c].sum())             # the negative taps meet -32768
    assert neg > 0 and abs(int(acc[t, c])) == want and want > 2 ** 31
    assert np.abs(acc).max() == want


@pytest.mark.parametrize("W", WS)
def test_identities_with_the_s8_model(W):
    """256 x at shift s + 8, and x sign-extended at shift s, give the s8 splitter's rows and clips."""
    n = 2 * W * spm.GEOM[MODE][1]
    wide8 = np.random.default_rng(160 + W).integers(-128, 128, (2, 1, n), dtype=np.int8)
    wide8[:, :, 3::991] = -128
    a8 = spm.sums(MODE, W, wide8)
    a256 = s16.sums(MODE, W, s16.widen256(wide8))
    aext = s16.sums(MODE, W, s16.sign_extend(wide8))
    assert np.array_equal(a256, 256 * a8) and np.array_equal(aext, a8)
    clipped = False
    for s in (1, spm.SHIFT_DEFAULT[W] - 4, spm.SHIFT_DEFAULT[W], 24):
        ref, ref_clips = spm.finish_all(a8, s)
        clipped |= bool(ref_clips.any())
        rows, clips, peaks = s16.finish_all(a256, s + 8)
        assert np.array_equal(rows, ref) and np.array_equal(clips, ref_clips), (W, s, "x 256")
        assert np.array_equal(peaks, 256 * np.abs(a8).reshape(2, 1, -1, 2 * W - 1, 2).max(axis=(0, 2, 4)))
        rows, clips, _ = s16.finish_all(aext, s)
        assert np.array_equal(rows, ref) and np.array_equal(clips, ref_clips), (W, s, "sign-extended")
    assert clipped                                                  # the clip counters were really compared


def test_cut_independence():
    """The sums of a capture do not depend on where it is cut into pieces (the history carries T - 1 samples)."""
    W, b = 4, 1000
    x = np.random.default_rng(5).integers(-32768, 32768, 2 * W * b, dtype=np.int16)
    whole = s16.Split16Model(MODE, W).flipped(x, b)
    for cuts in ((1, 999), (15, 16, 17, 952), (63, 64, 65, 808), (500, 499, 1)):
        m = s16.Split16Model(MODE, W)
        parts, at = [], 0
        for n in cuts:
            parts.append(m.flipped(x[2 * W * at:2 * W * (at + n)], n))
            at += n
        assert at == b and np.array_equal(np.concatenate(parts), whole), cuts


def _gain_blocks(W):
    """Flipped sums [4 cases][b][2 R] of short captures: full-range random, a weak one (|x| <= 40), full scale
    with random signs, and silence."""
    b = 512
    rng = np.random.default_rng(900 + W)
    caps = [rng.integers(-32768, 32768, 2 * W * b, dtype=np.int16),
            rng.integers(-40, 41, 2 * W * b, dtype=np.int16),
            np.where(rng.integers(0, 2, 2 * W * b) == 1, 32767, -32768).astype(np.int16),
            np.zeros(2 * W * b, np.int16)]
    return [s16.Split16Model(MODE, W).flipped(c, b) for c in caps]


@pytest.mark.parametrize("target", (1, 90, 127))
@pytest.mark.parametrize("W", WS)
def test_gain_rule_properties(W, target):
    for case, acc in enumerate(_gain_blocks(W)):
        _, _, peaks = s16.finish(acc, s16.SHIFT_DEFAULT[W])
        shifts = s16.shifts_for(peaks, target, W)
        rows, clips, peaks2 = s16.finish(acc, shifts)
        assert np.array_equal(peaks, peaks2)                        # the peaks do not depend on the shifts
        assert not clips.any(), (W, target, case)                   # 1: nothing clips
        exc = np.abs(rows.astype(np.int64) - 128).max(axis=1)
        assert exc.max() <= target
        for r in range(2 * W - 1):                                  # 2: a row the rule gave s > 1 is at least half used
            if shifts[r] > 1 and peaks[r] > 0:
                assert exc[r] >= target // 2, (W, target, case, r, int(peaks[r]), int(shifts[r]))
        if case == 3:
            assert (shifts == s16.SHIFT_DEFAULT[W]).all() and (rows == 128).all()
        if case == 1 and target >= 90:                              # 40 max_col sum |e| < 2^23: s <= 17 for every W
            assert (shifts < s16.SHIFT_DEFAULT[W] - 4).all()        # the weak capture does get more gain


def test_gain_rule_is_minimal():
    for target in (1, 90, 127):
        for peak in (1, 2, 89, 90, 91, 180, 181, 12345, 2 ** 31, 6089736192, 2 ** 33):
            s = s16.shift_for(peak, target, 8)
            assert 1 <= s <= 33 and s16.rnd(peak, s) <= target
            assert s == 1 or s16.rnd(peak, s - 1) > target


def test_library_shift_for(pkg):
    L = pkg.lib()
    peaks = [0, 1] + [v for k in range(1, 34) for v in (2 ** k - 1, 2 ** k, 2 ** k + 1)]
    for W in WS:
        for target in (1, 90, 127):
            for p in peaks:
                assert L.sdr_split16_shift_for(p, target, W) == s16.shift_for(p, target, W), (W, target, p)
        assert pkg.split16_shift_for(0, W=W) == s16.SHIFT_DEFAULT[W]
        assert pkg.split16_shift_for(12345, W=W) == s16.shift_for(12345, 90, W)
    for bad in ((1, 0, 8), (1, 128, 8), (1, 90, 5), (-1, 90, 8)):
        assert L.sdr_split16_shift_for(*bad) == -1
    with pytest.raises(pkg.SdrError):
        pkg.split16_shift_for(1, 128, W=8)
