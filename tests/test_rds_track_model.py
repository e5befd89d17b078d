"""CPU: the RDS symbol tracker's definition (tests/rds_track_model.py) on rows made here: ideal chips from
every starting phase, a clock that walks, an acquisition on the wrong half, call-cut invariance, poison and
the int32 bounds. No GPU, no DSP."""
from __future__ import annotations

import numpy as np
import pytest

import rds_track_model as tm

S, B = tm.S, tm.B
ROW = 2836                                    # a block's rds_clean samples in mode 0


def _bits(seed: int, n: int) -> list:
    return [int(v) for v in np.random.Generator(np.random.PCG64(seed)).integers(0, 2, n)]


def _rows(x, n: int = ROW):
    return [x[i:i + n] for i in range(0, len(x), n)]


def _check_tail(ch, out, true_bits, lead: int, count: int | None = None):
    """The last `count` emitted bits (all but the first by default: that one has no previous raw bit) are
    the true ones; `lead` = the index in the uncut chip stream of the tracker's sample 0, plus the samples
    taken out (minus those put in) since. The next bit's start must be on a bit boundary, within a sample."""
    pos = ch.t + lead
    idx = (pos + S) // B                      # the nearest boundary
    assert abs(pos - idx * B) <= 1, (pos % B, "not on a bit boundary")
    count = len(out) - 1 if count is None else count
    assert count > 0 and idx <= len(true_bits)
    assert out[len(out) - count:] == true_bits[idx - count:idx]


# ---------------------------------------------------------------- ideal rows
def test_ideal_rows_from_every_phase():
    true_bits = _bits(1, 120)
    x = tm.chips(true_bits, 1.0)
    for p in range(B):
        out, ch = tm.track(_rows(x[p:]))
        st = ch.stats()
        assert st["locked"] == 1 and st["acquired"] == 1 and st["half_moves"] == 0 and st["moves"] == 0, (p, st)
        assert st["phase"] == (-p) % B, p
        assert len(out) >= 120 - tm.A - 3, (p, len(out))
        _check_tail(ch, out, true_bits, p)
        assert st["level"] == tm.T * B * (1 << tm.QSHIFT)


# ---------------------------------------------------------------- the walk
@pytest.mark.parametrize("doubled", [False, True])
def test_walk_is_followed(doubled):
    """One sample dropped (or doubled) every block of 2836, as the 247/640 resampler's 0.64 samples a block
    and a transmitter off by some ppm add up to: no bit is lost, and the phase goes the way the samples went."""
    nblocks, start = 30, 5
    true_bits = _bits(2, nblocks * ROW // B + 40)
    x = tm.chips(true_bits, 0.75)[17:]
    at = np.arange(start, nblocks) * ROW + 1000
    x = np.insert(x, at, x[at]) if doubled else np.delete(x, at)
    out, ch = tm.track(_rows(x[:nblocks * ROW]))
    d = len(at)
    st = ch.stats()
    assert st["half_moves"] == 0 and st["moves"] == d, st
    _check_tail(ch, out, true_bits, 17 + (-d if doubled else d))
    want = ((-17) % B + (d if doubled else -d)) % B
    assert st["phase"] == want, (st, want)


# ---------------------------------------------------------------- the wrong half
def test_wrong_half_is_left():
    """All-zero bits make the two alignments equal, the first maximum is then the smaller residue: with the
    right one at 50 acquisition takes 11. The half check moves it once data comes."""
    true_bits = [0] * (tm.A + 4) + _bits(3, 300)
    p = (-50) % B
    x = tm.chips(true_bits, 0.5)[p:]
    calls = _rows(x)
    ch = tm.Channel()
    nb0, first = ch.call(calls[0])
    assert ch.locked and ch.stats()["phase"] == 50 - S and nb0 > 0
    out = list(first)
    for r in calls[1:]:
        out += ch.call(r)[1]
    st = ch.stats()
    assert st["half_moves"] == 1 and st["phase"] == 50 and st["acquired"] == 1, st
    _check_tail(ch, out, true_bits, p, count=150)


# ---------------------------------------------------------------- call-cut invariance
def _feed(x, sizes, **opts):
    ch, out, at, ncalls = tm.Channel(**opts), [], 0, 0
    for n in sizes:
        n = min(n, len(x) - at)
        nb, bits = ch.call(x[at:at + n])
        assert nb == len(bits)
        out += bits
        at += n
        ncalls += 1
        if at == len(x):
            break
    assert at == len(x)
    return out, ch.state()


def test_call_cut_invariance():
    x, _ = tm.noise_rows(4, 8 * ROW)
    x = np.delete(x, [3 * ROW + 500, 6 * ROW + 7])               # the clock steps twice
    want, state = _feed(x, [ROW] * 8)
    assert len(want) > 200 and state[2] == 1
    assert dict(zip(tm.STATS, state[-len(tm.STATS):]))["moves"] >= 1
    plans = {"1000+1836": [1000, 1836] * 8, "77/78/79": [77, 78, 79] * 100, "ones": [1] * len(x),
             "zeros between": [0, ROW, 0, 0, 1, 0, 999, 0] * 8, "max": [tm.MAX_N, 0, tm.MAX_N],
             "uneven": [1, 77, 2836, 0, 78, 1000, 79, 4097, 3071, 3073] * 3}
    for name, sizes in plans.items():
        got, st = _feed(x, sizes)
        assert got == want, name
        assert st == state, name


OPTION_SETS = (dict(acquire_bits=1), dict(acquire_bits=64), dict(half_bits=16), dict(half_bits=32), dict(qshift=0),
               dict(qshift=15))


@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_call_cut_invariance_under_options(opts):
    """Every option away from its default, on a stream that has to be rounded and whose clock steps: the cut
    into calls changes neither the bits nor the state, at the lengths around the kernel's chunk and carry too."""
    n = sum(tm.BOUNDARY_SIZES)
    q = opts.get("qshift", tm.QSHIFT)
    x = np.delete(tm.off_grid(7, n + 2, qshift=q), [3 * ROW + 500, 6 * ROW + 7])
    assert np.array_equal(tm.quantise(x, q), np.delete(tm.quantise(tm.off_grid(7, n + 2)), [3 * ROW + 500, 6 * ROW + 7]))
    want, state = _feed(x, [ROW] * (n // ROW + 1), **opts)
    st = dict(zip(tm.STATS, state[-len(tm.STATS):]))
    assert len(want) > 700 and st["locked"] == 1 and st["moves"] >= 1, st
    plans = {"uneven": [1, 77, 2836, 0, 78, 1000, 79, 4097, 3071, 3073] * 5, "boundaries": tm.boundary_plan(8, 17)}
    assert sum(plans["uneven"]) >= n and sum(plans["boundaries"]) == n
    for name, sizes in plans.items():
        got, st = _feed(x, sizes, **opts)
        assert got == want, name
        assert st == state, name


def test_a_shorter_half_check_leaves_the_wrong_half_earlier():
    left = {}
    for hb in (16, 64):
        ch, x = tm.Channel(half_bits=hb), tm.wrong_half(3, 12 * ROW)
        for k in range(0, len(x), B):
            ch.call(x[k:k + B])
            if ch.half_moves and hb not in left:
                left[hb] = k
        st = ch.stats()
        assert st["locked"] == 1 and st["half_moves"] == 1 and st["phase"] == 50 and st["acquired"] == 1, (hb, st)
    assert left[16] < left[64], left


@pytest.mark.parametrize("value", [0.0, 0.25, -0.0])
@pytest.mark.parametrize("acquire_bits", [1, 32, 64])
def test_silence_locks_at_phase_zero_and_gives_zero_bits(value, acquire_bits):
    """Every E is equal, so the first maximum is residue 0; every correlator is 0, so nothing moves."""
    ch = tm.Channel(acquire_bits=acquire_bits)
    need = (acquire_bits + 1) * B - 1                              # the last acquisition position's last sample
    x = np.full(need + 5 * ROW, value, np.float32)
    assert ch.call(x[:need - 1]) == (0, []) and not ch.locked
    assert ch.call(x[need - 1:need]) == (0, []) and ch.locked and ch.t == acquire_bits * B
    out = []
    for r in _rows(x[need:]):
        out += ch.call(r)[1]
    assert len(out) == (len(x) - 1) // B - acquire_bits and not any(out)
    assert ch.stats() == dict(locked=1, phase=0, bits=len(out), moves=0, half_moves=0, resets=0, level=0, acquired=1)


def test_the_stream_builders_are_what_they_say():
    k = np.float32(1 << tm.QSHIFT)
    x = tm.off_grid(9, 20000)
    y = x.astype(np.float64) * float(k)
    assert np.mean(y != np.rint(y)) >= 0.9
    assert np.sum(np.abs(y - np.floor(y) - 0.5) == 0) >= 50 and np.isfinite(x).all()
    for v in tm.OFF_GRID_SPECIALS:
        assert np.sum(x.view(np.uint32) == np.float32(v).view(np.uint32)) >= 4, v
    for qs in (0, 15):
        assert np.array_equal(tm.quantise(tm.off_grid(9, 20000, qshift=qs), qs), tm.quantise(x))
    base = tm.noise_rows(21, 4003)[0]                              # three steps in 4000 samples
    d, i = tm.walking(21, 4000, 1247, False), tm.walking(21, 4000, 1249, True)
    assert np.array_equal(d[:1246], base[:1246]) and np.array_equal(d[1246:2492], base[1247:2493])
    assert np.array_equal(i[:1249], base[:1249]) and i[1249] == base[1248] and np.array_equal(i[1250:2498], base[1249:2497])
    plan = tm.boundary_plan(1)
    assert len(plan) == 40 and set(plan) == set(tm.BOUNDARY_SIZES)


# ---------------------------------------------------------------- poison and reset
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_poison_restarts_the_stream(bad):
    true_bits = _bits(5, 300)
    x = tm.chips(true_bits, 1.0)[30:]
    ch = tm.Channel()
    nb, bits = ch.call(x[:ROW])
    assert nb > 0 and ch.locked
    before = ch.stats()
    row = x[ROW:2 * ROW].copy()
    row[ROW - 1] = bad
    assert ch.call(row) == (tm.NBITS_POISONED, [])
    st = ch.stats()
    assert (st["locked"], st["phase"], st["level"], st["resets"]) == (0, 0, 0, 1)
    assert (st["bits"], st["acquired"]) == (before["bits"], 1) and ch.n == 0 and not ch.carry.any() and not ch.E.any()
    assert ch.call(x[:0]) == (0, [])                               # n = 0 is legal and changes nothing
    out = []
    for r in _rows(x[2 * ROW:]):
        out += ch.call(r)[1]
    st = ch.stats()
    assert st["locked"] == 1 and st["acquired"] == 2 and st["resets"] == 1
    _check_tail(ch, out, true_bits, 30 + 2 * ROW)
    ch.reset()
    assert ch.stats() == dict.fromkeys(tm.STATS, 0)


# ---------------------------------------------------------------- bounds
def test_quantisation():
    k = float(1 << tm.QSHIFT)
    x = np.array([0.0, 0.5 / k, 1.5 / k, 2.5 / k, -0.5 / k, -1.5 / k, 31.9985, 32.0, 40.0, -40.0, 3e38, -3e38, 1e-40],
                 np.float32)
    assert tm.quantise(x).tolist() == [0, 0, 2, 2, 0, -2, 32766, 32767, 32767, -32767, 32767, -32767, 0]


def test_full_scale_overflows_nothing():
    """+-32767 everywhere (the clamp), in calls of the longest accepted length: the model asserts the int32
    bound of every prefix sum, correlator and accumulator as it goes."""
    true_bits = [0] * 80 + _bits(6, 2 * tm.MAX_N // B)             # long constant runs: the largest sums
    x = tm.chips(true_bits, 1000.0)[(-50) % B:]
    out, ch = tm.track(_rows(x[:2 * tm.MAX_N], tm.MAX_N), acquire_bits=64)
    st = ch.stats()
    assert st["locked"] and st["level"] == tm.T * B * tm.QMAX and st["half_moves"] == 1
    assert max(len(out), 0) <= 2 * tm.MAX_BITS
    with pytest.raises(ValueError):
        tm.Channel().call(np.zeros(tm.MAX_N + 1, np.float32))
    for bad in (dict(qshift=16), dict(qshift=-1), dict(acquire_bits=0), dict(acquire_bits=65), dict(half_bits=8),
                dict(half_bits=40), dict(half_bits=80)):
        with pytest.raises(ValueError):
            tm.Channel(**bad)


def test_the_bound_on_bits_per_call_is_tight():
    """Bits are at least B - 1 samples apart (one early step every T bits): MAX_N samples hold at most
    MAX_BITS bits, and the arithmetic of that bound is the header's."""
    assert tm.MAX_N == 19712 and (tm.MAX_N - 1) // (B - 1) + 1 == tm.MAX_BITS and tm.MAX_N // (B - 1) + 1 > tm.MAX_BITS
    assert (tm.CARRY + tm.MAX_N) * tm.QMAX < 1 << 31 and B * tm.QMAX * 64 < 1 << 31
