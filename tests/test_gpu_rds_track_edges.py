"""GPU: the RDS symbol tracker (k_rds_track of sdr_rds_track.hip) against the model of tests/rds_track_model.py
where tests/test_gpu_rds_track.py does not go: options away from their defaults (an acquisition longer than a
chunk), call lengths at every chunk and carry boundary on both staging paths, non-finite samples of every
kind and place, samples the quantisation has to round, silence, the cap on a call's bits, and the host
surface (reset, queued calls on a stream, two trackers, a second block of channels). Everything is compared
exactly, after every call: nbits, bits[:nbits] and the eight stats fields. What each test needs of its input
(that it locks where it should, that it has ties, that the clock walks) is asserted on the model."""
from __future__ import annotations

import copy

import numpy as np
import pytest

import rds_track_model as tm

pytestmark = pytest.mark.gpu

S, B, ROW, MAX_N, CHUNK = tm.S, tm.B, 2836, tm.MAX_N, tm.CHUNK
STRIDE = MAX_N + 4                                  # a multiple of 4: rows are all 16-byte aligned or none is


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _stats_row(rec) -> dict:
    return {k: int(rec[k]) for k in tm.STATS}


def _compare(k, models, rows, n, nbits, bits, stats) -> list:
    """One call of every channel's model on rows[c][:n] against what the GPU gave; the models' (nbits, bits)."""
    out = []
    for c, m in enumerate(models):
        nb, want = m.call(rows[c][:n])
        assert int(nbits[c]) == nb, (k, c, n, int(nbits[c]), nb)
        if nb > 0:
            assert bits[c, :nb].tolist() == want, (k, c, n)
        if stats is not None:
            assert _stats_row(stats[c]) == m.stats(), (k, c, n)
        out.append((nb, want))
    return out


def _device_rows(torch, nch: int, shift: int):
    """[nch][STRIDE] f32 on the device from a base `shift` floats past a 16-byte boundary: shift 0 stages every
    row with 16-byte loads, shift 1 every row with scalar loads."""
    flat = torch.zeros(nch * STRIDE + 8, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    d_row = flat[shift:shift + nch * STRIDE].view(nch, STRIDE)
    aligned = sum(1 for c in range(nch) if (d_row.data_ptr() + 4 * STRIDE * c) % 16 == 0)
    assert aligned == (nch if shift == 0 else 0)
    return d_row


def _run(torch, trk, d_row, models, x, calls, at: int = 0) -> list:
    """The calls, one after the other from x[:, at:], each compared; every call's model results."""
    seen = []
    for k, n in enumerate(calls):
        rows = np.ascontiguousarray(x[:, at:at + n])
        assert rows.shape[1] == n
        at += n
        if n:
            d_row[:, :n].copy_(torch.from_numpy(rows))
        d_nb, d_bits = trk.feed(d_row, n)
        stats = trk.stats()
        seen.append(_compare(k, models, rows, n, d_nb.cpu().numpy(), d_bits.cpu().numpy(), stats))
    return seen


def _silent(m, nbits_and_bits) -> bool:
    st = m.stats()
    return (st["locked"], st["phase"], st["level"], st["moves"], st["half_moves"]) == (1, 0, 0, 0, 0) and st["bits"] > 0 \
        and not any(any(b) for _, b in nbits_and_bits)


# ---------------------------------------------------------------- a. options
CALLS_A = (MAX_N, 1, 3073, 78, 2836, 3072, 0, 5000)
CASES_A = [(dict(acquire_bits=1), CALLS_A), (dict(acquire_bits=64), CALLS_A), (dict(half_bits=16), CALLS_A),
           (dict(half_bits=32), CALLS_A), (dict(qshift=0), CALLS_A), (dict(qshift=15), CALLS_A),
           (dict(qshift=0, acquire_bits=64, half_bits=16), CALLS_A), (dict(acquire_bits=64), (3000,) * 12)]


def option_streams(opts: dict, total: int) -> np.ndarray:
    """Noisy chips from 23 samples into a bit, the wrong-half stream of this acquisition length, off_grid; scaled
    so that another qshift quantises to the same stream."""
    q, a = opts.get("qshift", tm.QSHIFT), opts.get("acquire_bits", tm.A)
    return np.stack([tm.for_qshift(tm.noise_rows(31, total + 23)[0][23:], q), tm.for_qshift(tm.wrong_half(32, total, a), q),
                     tm.off_grid(33, total, qshift=q)])


def check_options_case(opts: dict, calls, models, seen):
    """What the case needs of the model's run."""
    final = [m.stats() for m in models]
    assert all(s["locked"] == 1 and s["resets"] == 0 for s in final), final
    assert final[1]["half_moves"] == 1 and final[1]["phase"] == 50, final[1]
    if opts.get("acquire_bits") == 64:
        assert 64 * B > CHUNK                                   # the acquisition cannot end in a call's first chunk
        first = [nb for nb, _ in seen[0]]
        if calls[0] == MAX_N:
            assert all(nb > 0 for nb in first), first           # from reset, locked in the second chunk
        else:
            assert calls[0] + B <= 64 * B and first == [0, 0, 0]    # still acquiring after the first call


@pytest.mark.parametrize("opts,calls", CASES_A, ids=lambda v: ",".join(f"{k}={w}" for k, w in v.items()) if isinstance(v, dict)
                         else f"{len(v)}calls")
def test_options_against_the_model(pkg, torch_cuda, opts, calls):
    torch = torch_cuda
    x = option_streams(opts, sum(calls))
    models = [tm.Channel(**opts) for _ in range(3)]
    trk = pkg.RdsTracker(3, **opts)
    seen = _run(torch, trk, _device_rows(torch, 3, 0), models, x, calls)
    check_options_case(opts, calls, models, seen)
    trk.close()


# ---------------------------------------------------------------- b. chunk and carry boundaries
def boundary_streams(total: int) -> np.ndarray:
    return np.stack([tm.noise_rows(41, total + 61)[0][61:], tm.off_grid(42, total), tm.walking(43, total, 1247, False),
                     np.zeros(total, np.float32)])


def check_boundary_run(models, seen):
    final = [m.stats() for m in models]
    assert all(s["locked"] == 1 and s["acquired"] == 1 for s in final), final
    assert final[2]["moves"] >= 40 and final[0]["bits"] > 1000 and final[0]["phase"] == B - 61, final
    assert _silent(models[3], [call[3] for call in seen])


@pytest.mark.parametrize("shift", [0, 1])
def test_every_length_at_a_chunk_or_carry_boundary(pkg, torch_cuda, shift):
    """Forty calls of the lengths 0..5, around TRK_CARRY, around one and two chunks and the longest two, once
    on 16-byte aligned rows (n < 4 leaves the vector path nothing) and once on rows one float past that."""
    torch = torch_cuda
    plan = tm.boundary_plan(65)                     # this seed: six calls of 3 to 121 samples come first, acquiring
    assert len(plan) == 40 and all(n in plan for n in tm.BOUNDARY_SIZES) and sum(plan[:6]) + B <= tm.A * B
    x = boundary_streams(sum(plan))
    models = [tm.Channel() for _ in range(4)]
    trk = pkg.RdsTracker(4)
    seen = _run(torch, trk, _device_rows(torch, 4, shift), models, x, plan)
    check_boundary_run(models, seen)
    trk.close()


# ---------------------------------------------------------------- c. poison
def _patterns() -> np.ndarray:
    """The six non-finite values as int32 bit patterns (no float arithmetic touches them: it would quiet the
    signalling ones): nan, -nan, +inf, -inf, a signalling NaN, a negative NaN with the smallest payload."""
    f = np.array([np.nan, -np.nan, np.inf, -np.inf], np.float32).view(np.uint32)
    p = np.concatenate([f, np.array([0x7FA00000, 0xFF800001], np.uint32)])
    assert p[0] >> 31 == 0 and p[1] >> 31 == 1 and (p[0] & 0x7FFFFFFF) > 0x7F800000 and (p[1] & 0x7FFFFFFF) > 0x7F800000
    assert not np.isfinite(p.view(np.float32)).any()
    return p.view(np.int32)


POISON_CALLS = (1000, 1003, ROW, 2837, 2838, MAX_N, 1, 3075, ROW, MAX_N, 2839, 3075, ROW, ROW, 1000)
# call -> {channel: the index of its bad sample}; channel 0 stays clean
POISON_AT = {1: {5: 1001},                       # still acquiring (2003 samples < A * B), in the scalar tail of an aligned row
             3: {1: 0},
             4: {2: 2837},                       # n - 1
             5: {3: CHUNK + 17},                 # the second chunk, tracking
             6: {4: 0},                          # a call of one sample
             7: {4: CHUNK + 1},                  # the second chunk, and the first alone would complete the acquisition
             9: {1: 6 * CHUNK + 5},              # the last chunk of the longest call
             11: {1: 3074, 2: 0, 3: CHUNK, 4: 1500, 5: CHUNK - 1}}    # every channel but 0 at once
# the bad sample is behind the first chunk: a kernel that used the chunks before it would show it in the stats
POISON_BEHIND = ((5, 3), (7, 4), (9, 1))


def poison_streams(total: int) -> np.ndarray:
    """Noisy chips from six phases; channels 1 and 3 walk, so that every round of theirs counts a move."""
    x = [tm.noise_rows(60 + c, total + 13 * c)[0][13 * c:] for c in range(6)]
    x[1], x[3] = tm.walking(61, total, 1247, False), tm.walking(63, total, 1249, True)
    return np.stack(x)


def check_poison_plan():
    ev = [(k, c, i, POISON_CALLS[k]) for k, d in sorted(POISON_AT.items()) for c, i in sorted(d.items())]
    assert all(0 <= i < n and c != 0 for _, c, i, n in ev) and {c for _, c, _, _ in ev} == {1, 2, 3, 4, 5}
    assert any(i == 0 for _, _, i, _ in ev) and any(i == n - 1 for _, _, i, n in ev)
    assert any(n % 4 and n - n % 4 <= i < n - 1 for _, _, i, n in ev)              # the vec4 path's scalar tail
    assert any(CHUNK <= i < 2 * CHUNK for _, _, i, _ in ev)
    assert any(n == MAX_N and i >= MAX_N - MAX_N % CHUNK for _, _, i, n in ev)
    assert any(n == 1 for _, _, _, n in ev) and len(POISON_AT[11]) == 5
    assert sum(POISON_CALLS[:2]) + B <= tm.A * B                                     # call 1 meets a channel that acquires
    assert {n % 4 for n in POISON_CALLS} == {0, 1, 2, 3}                             # the slack behind every n mod 4
    return ev


@pytest.mark.parametrize("shift", [0, 1])
def test_poison_of_every_kind_and_place(pkg, torch_cuda, shift):
    """One tracker gets the poisoned rows with four NaNs in the slack behind every call's n, a second one the
    clean rows with zeros behind them: channel 0 of the two is the same to the bit, the poisoned calls give
    SDR_NBITS_POISONED, resets + 1 and nothing else, and every channel acquires again as the model does."""
    torch = torch_cuda
    ev = check_poison_plan()
    pat = _patterns()
    value = {(k, c): pat[(e + 3 * shift) % 6] for e, (k, c, _, _) in enumerate(ev)}
    assert {int(v) for v in value.values()} == {int(v) for v in pat}
    nch = 6
    x = poison_streams(sum(POISON_CALLS))
    models, clean_models = [tm.Channel() for _ in range(nch)], [tm.Channel() for _ in range(nch)]
    trk, ref = pkg.RdsTracker(nch), pkg.RdsTracker(nch)
    d_row, d_clean = _device_rows(torch, nch, shift), _device_rows(torch, nch, shift)
    ref_nb = torch.zeros(nch, dtype=torch.int32, device="cuda")
    ref_bits = torch.zeros(nch, 256, dtype=torch.uint8, device="cuda")
    at, before = 0, trk.stats()
    for k, n in enumerate(POISON_CALLS):
        clean = np.ascontiguousarray(x[:, at:at + n])
        at += n
        rows = clean.copy()
        for c, i in POISON_AT.get(k, {}).items():
            rows.view(np.int32)[c, i] = value[k, c]
        assert np.array_equal(rows[0].view(np.int32), clean[0].view(np.int32))
        for c in (c for kk, c in POISON_BEHIND if kk == k):
            assert POISON_AT[k][c] >= CHUNK
            probe = copy.deepcopy(models[c])
            probe.call(clean[c][:CHUNK])
            was, now = models[c].stats(), probe.stats()
            assert (was["moves"], was["acquired"]) != (now["moves"], now["acquired"]), (k, c)
        d_row[:, :n].copy_(torch.from_numpy(rows))
        d_row[:, n:n + 4] = float("nan")                      # behind the call's samples: not the call's
        d_clean[:, :n].copy_(torch.from_numpy(clean))
        d_nb, d_bits = trk.feed(d_row, n)
        stats = trk.stats()
        ref.feed(d_clean, n, nbits=ref_nb, bits=ref_bits)
        ref_stats = ref.stats()
        nb, bits = d_nb.cpu().numpy(), d_bits.cpu().numpy()
        _compare(k, models, rows, n, nb, bits, stats)
        cnb, cbits = ref_nb.cpu().numpy(), ref_bits.cpu().numpy()
        _compare(k, clean_models, clean, n, cnb, cbits, ref_stats)
        assert nb[0] == cnb[0] and np.array_equal(bits[0, :max(nb[0], 0)], cbits[0, :max(nb[0], 0)]), k
        assert _stats_row(stats[0]) == _stats_row(ref_stats[0]), k
        for c in range(1, nch):
            if c in POISON_AT.get(k, {}):
                assert nb[c] == pkg.SDR_NBITS_POISONED == tm.NBITS_POISONED, (k, c)
                want = dict(_stats_row(before[c]), locked=0, phase=0, level=0, resets=int(before[c]["resets"]) + 1)
                assert _stats_row(stats[c]) == want, (k, c)      # bits, acquired, moves and half_moves as before
            else:
                assert nb[c] >= 0 and stats[c]["resets"] == before[c]["resets"], (k, c)
        before = stats
    final = [m.stats() for m in models]
    assert all(s["locked"] == 1 for s in final) and final[0]["resets"] == 0 and final[0]["acquired"] == 1, final
    assert [s["resets"] for s in final[1:]] == [3, 2, 2, 3, 2] and [s["acquired"] for s in final[1:]] == [4, 3, 3, 3, 2], final
    trk.close()
    ref.close()


# ---------------------------------------------------------------- d. quantisation and silence
CALLS_D = (ROW,) * 4 + (MAX_N,)


def quantisation_streams(total: int) -> np.ndarray:
    """off_grid; zero, 0.25 and -0.0 throughout; off_grid 200 times as large, beyond the clamp but for its ties and
    small specials (its +-3e38 stay as they are: times 200 they would be inf), the last two rounds without those."""
    return np.stack([tm.off_grid(51, total), np.zeros(total, np.float32), np.full(total, 0.25, np.float32),
                     np.full(total, -0.0, np.float32),
                     tm.off_grid(52, total, sigma_q=100, gain=200.0, quiet_tail=(2 * tm.T + 1) * B)])


def check_quantisation_run(x, models, seen):
    y = x[0].astype(np.float64) * (1 << tm.QSHIFT)
    assert np.mean(y != np.rint(y)) >= 0.9 and np.sum(np.abs(y - np.floor(y)) == 0.5) >= 50
    assert np.signbit(x[3]).all() and np.isfinite(x).all()
    big = np.abs(x[4].astype(np.float64)) * (1 << tm.QSHIFT)
    assert 0.95 < np.mean(big > tm.QMAX) < 1 and np.sum(np.abs(x[4]) == np.float32(3e38)) == 8
    final = [m.stats() for m in models]
    assert all(s["locked"] == 1 and s["resets"] == 0 for s in final), final
    for c in (1, 2, 3):
        assert _silent(models[c], [call[c] for call in seen]), c
    assert final[4]["level"] == tm.T * B * tm.QMAX and final[0]["bits"] > 300


def test_rounding_clamping_and_silence(pkg, torch_cuda):
    torch = torch_cuda
    x = quantisation_streams(sum(CALLS_D))
    models = [tm.Channel() for _ in range(5)]
    trk = pkg.RdsTracker(5)
    seen = _run(torch, trk, _device_rows(torch, 5, 0), models, x, CALLS_D)
    check_quantisation_run(x, models, seen)
    trk.close()


# ---------------------------------------------------------------- e. the bit cap
def cap_streams() -> np.ndarray:
    return np.stack([tm.walking(21, 3 * MAX_N, 1247, False, 300, 60), tm.walking(22, 3 * MAX_N, 1249, True, 300, 60)])


def check_cap_run(models, seen):
    fast = [call[0][0] for call in seen]
    assert fast[1] >= 253 and fast[2] >= 253 and max(fast) <= tm.MAX_BITS, fast      # B - 1 samples a bit
    assert all(m.stats()["moves"] >= 40 and m.stats()["half_moves"] == 0 for m in models), [m.stats() for m in models]


def test_a_call_near_the_bit_cap_stays_in_its_row(pkg, torch_cuda):
    """The clock steps early every round: 253 bits of the 256 a call may give, into rows exactly 256 wide
    between two guard rows."""
    torch = torch_cuda
    x = cap_streams()
    models = [tm.Channel() for _ in range(2)]
    trk = pkg.RdsTracker(2)
    d_row = _device_rows(torch, 2, 0)
    guarded = torch.full((4, tm.MAX_BITS), 7, dtype=torch.uint8, device="cuda")
    d_bits = guarded[1:3]
    d_nb = torch.full((2,), -9, dtype=torch.int32, device="cuda")
    seen = []
    for k in range(3):
        rows = np.ascontiguousarray(x[:, k * MAX_N:(k + 1) * MAX_N])
        d_row[:, :MAX_N].copy_(torch.from_numpy(rows))
        trk.feed(d_row, MAX_N, nbits=d_nb, bits=d_bits)
        stats = trk.stats()
        seen.append(_compare(k, models, rows, MAX_N, d_nb.cpu().numpy(), d_bits.cpu().numpy(), stats))
        g = guarded.cpu().numpy()
        assert (g[0] == 7).all() and (g[3] == 7).all(), k
        if k == 0:
            assert all((g[1 + c, seen[0][c][0]:] == 7).all() for c in range(2))      # nothing behind nbits either
    check_cap_run(models, seen)
    trk.close()


# ---------------------------------------------------------------- f. the host surface
def test_reset_with_a_second_block_of_channels(pkg, torch_cuda):
    """257 channels: the second 256-thread block of the stats kernel and the tail of the reset kernel's grid.
    After reset() every channel is a fresh tracker."""
    torch = torch_cuda
    nch = 257
    x = np.stack([tm.noise_rows(1000 + c, 4 * ROW)[0] for c in range(nch)])
    trk = pkg.RdsTracker(nch)
    d_row = torch.zeros(nch, ROW, dtype=torch.float32, device="cuda")
    models = [tm.Channel() for _ in range(nch)]
    _run(torch, trk, d_row, models, x, (ROW, ROW))
    assert all(m.locked and m.bits > 30 for m in models)
    trk.reset()
    assert all(_stats_row(r) == dict.fromkeys(tm.STATS, 0) for r in trk.stats())
    models = [tm.Channel() for _ in range(nch)]
    _run(torch, trk, d_row, models, x, (ROW, ROW), at=2 * ROW)
    assert all(m.locked and m.bits > 30 and m.acquired == 1 for m in models)
    trk.close()


def test_eight_calls_queued_on_a_stream(pkg, torch_cuda):
    """No host synchronisation between the calls: the state is handed from kernel to kernel in stream order."""
    torch = torch_cuda
    nch, calls = 4, (ROW, 1, 3073, 0, 6145, 78, ROW, 5000)
    x = np.stack([tm.noise_rows(70, sum(calls))[0], tm.off_grid(71, sum(calls)), tm.walking(72, sum(calls), 1247, False),
                  tm.wrong_half(73, sum(calls))])
    cuts = np.concatenate([[0], np.cumsum(calls)])
    rows = [np.ascontiguousarray(x[:, cuts[k]:cuts[k + 1]]) for k in range(len(calls))]
    d_in = [torch.zeros(nch, max(n, 4), dtype=torch.float32, device="cuda") for n in calls]
    for k, n in enumerate(calls):
        if n:
            d_in[k][:, :n].copy_(torch.from_numpy(rows[k]))
    d_nb = [torch.full((nch,), -9, dtype=torch.int32, device="cuda") for _ in calls]
    d_bits = [torch.full((nch, 256), 7, dtype=torch.uint8, device="cuda") for _ in calls]
    trk = pkg.RdsTracker(nch)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for k, n in enumerate(calls):
        trk.feed(d_in[k], n, stream=stream, nbits=d_nb[k], bits=d_bits[k])
    stream.synchronize()
    models = [tm.Channel() for _ in range(nch)]
    for k, n in enumerate(calls):
        _compare(k, models, rows[k], n, d_nb[k].cpu().numpy(), d_bits[k].cpu().numpy(), None)
    stats = trk.stats(stream=stream)
    assert [_stats_row(r) for r in stats] == [m.stats() for m in models]
    assert all(m.locked for m in models) and sum(m.bits for m in models) > 4 * 200
    trk.close()


def test_two_trackers_with_different_options(pkg, torch_cuda):
    torch = torch_cuda
    nch, calls = 3, (ROW, 1000, 3073, ROW, ROW)
    opts = (dict(), dict(qshift=12, acquire_bits=16, half_bits=32))
    x = np.stack([tm.noise_rows(80, sum(calls))[0], tm.off_grid(81, sum(calls)), tm.wrong_half(82, sum(calls))])
    models = [[tm.Channel(**o) for _ in range(nch)] for o in opts]
    trks = [pkg.RdsTracker(nch, **o) for o in opts]
    d_row = _device_rows(torch, nch, 0)
    at = 0
    for k, n in enumerate(calls):
        rows = np.ascontiguousarray(x[:, at:at + n])
        at += n
        d_row[:, :n].copy_(torch.from_numpy(rows))
        out = [t.feed(d_row, n) for t in trks]                 # both queued before either is read
        for t, m, (d_nb, d_bits) in zip(trks, models, out):
            _compare(k, m, rows, n, d_nb.cpu().numpy(), d_bits.cpu().numpy(), t.stats())
    finals = [[m.stats() for m in ms] for ms in models]
    assert all(s["locked"] == 1 for f in finals for s in f) and finals[0] != finals[1], finals
    for t in trks:
        t.close()
