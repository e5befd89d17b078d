"""GPU: the RDS carrier-phase derotator (include/sdr_amd.h: sdr_rds_carrier_rotate and the kernel of
sdr_rds_carrier.hip) against the model of tests/rds_carrier_model.py. After the one quantisation everything is
integer, and the output is that integer times a power of two: rows and stats are compared exactly after every
call, for calls of every kind of length, alignment and option."""
from __future__ import annotations

import numpy as np
import pytest

import rds_carrier_model as cm

pytestmark = pytest.mark.gpu

W = cm.W
SIZES = (0, 1, 3, 2047, 2048, 2049, 3071, 3072, 3073, 3074, 3075, 6145, 19712)
SENTINEL = np.float32(-777.25)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _stats_row(rec) -> dict:
    return {k: int(rec[k]) for k in cm.STATS}


def _rows(torch, nch, stride, shift):
    """A [nch][stride] float32 view that starts `shift` floats past a 16-byte boundary."""
    flat = torch.zeros(nch * stride + 8, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    return flat[shift:shift + nch * stride].view(nch, stride)


def _streams(nch: int, total: int, qshift: int = cm.QSHIFT):
    """Channel c: chips turned by an angle of its own, all four quadrants among them, plus noise; one in three
    on the grid of 2^-qshift, one in three off it with exact ties and the clamp's specials, one in three driven
    far into the clamp."""
    xi, xq = np.empty((nch, total), np.float32), np.empty((nch, total), np.float32)
    base = {}
    for c in range(nch):
        kind, deg = c % 3, (c * 37.0 + 20.0) % 360.0 - 180.0
        key = (kind, c % 24)
        if key not in base:                           # 24 x 3 distinct streams; further channels get them rolled
            if kind == 0:
                base[key] = cm.rotated(300 + c, total, deg, qshift=qshift)[:2]
            else:
                base[key] = cm.off_grid(300 + c, total, deg, qshift=qshift, gain=1.0 if kind == 1 else 150.0)
        xi[c], xq[c] = (np.roll(v, c // 72 * 11) for v in base[key])
    return xi, xq


def _run_calls(torch, pkg, nch, sizes, shift, stride_pad=3, xs=None, poison=None, **opts):
    """The calls of `sizes` on a fresh handle and on fresh models; rows and stats compared after every call.
    poison: {call index: [(channel, row 0/1, index or -1 for n - 1, value)]}."""
    total = sum(sizes)
    xi, xq = xs if xs is not None else _streams(nch, total, opts.get("qshift", cm.QSHIFT))
    stride = max(sizes) + stride_pad
    d_i, d_q, d_o = (_rows(torch, nch, stride, shift) for _ in range(3))
    models = [cm.Channel(**opts) for _ in range(nch)]
    car = pkg.RdsCarrier(nch, **opts)
    at = 0
    for k, n in enumerate(sizes):
        ri, rq = xi[:, at:at + n].copy(), xq[:, at:at + n].copy()
        at += n
        for c, row, idx, val in (poison or {}).get(k, ()):
            (ri, rq)[row][c, idx if idx >= 0 else n + idx] = val
        # NaNs in the slack behind n: they are never read
        d_i.fill_(float("nan")), d_q.fill_(float("nan")), d_o.fill_(float(SENTINEL))
        if n:
            d_i[:, :n].copy_(torch.from_numpy(ri))
            d_q[:, :n].copy_(torch.from_numpy(rq))
        out = car.feed(d_i, d_q, n, out=d_o)
        stats = car.stats()
        got = out.cpu().numpy()
        for c in range(nch):
            want = models[c].call(ri[c], rq[c])
            assert np.array_equal(got[c, :n].view(np.uint32), want.view(np.uint32)), (k, c, n)
            assert _stats_row(stats[c]) == models[c].stats(), (k, c, n)
        assert np.all(got[:, n:] == SENTINEL), (k, n)
    car.close()
    return models


@pytest.mark.parametrize("nch,shift", [(3, 0), (3, 1), (257, 1)])
def test_every_call_length_and_alignment(pkg, torch_cuda, nch, shift):
    """Rows max(n) + 3 floats apart from a base `shift` floats past a 16-byte boundary: at shift 0 the first row
    of each buffer takes the 16-byte paths, at shift 1 with 257 channels a quarter of them do."""
    sizes = (2049, 0, 3073, 1, 2047, 19712, 3071, 3, 3075, 2048, 3072, 6145, 3074)
    assert set(sizes) == set(SIZES)
    models = _run_calls(torch_cuda, pkg, nch, sizes, shift)
    assert all(m.windows == sum(sizes) // W and m.phi != 0 for m in models)
    assert any(np.abs(m.y).max() == cm.QMAX for m in models)                 # the output clamp was reached


def test_every_row_16_byte_aligned(pkg, torch_cuda):
    """A stride that is a multiple of 4 floats: every row of all three buffers takes the 16-byte paths."""
    _run_calls(torch_cuda, pkg, 5, (2836, 2836, 3073, 2836, 6145, 2), 0, stride_pad=7)


@pytest.mark.parametrize("opts", [dict(qshift=0), dict(qshift=15), dict(qshift=7, avg_shift=0), dict(avg_shift=6),
                                  dict(avg_shift=1)], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_every_option_away_from_its_default(pkg, torch_cuda, opts):
    _run_calls(torch_cuda, pkg, 4, (2836, 2836, 1500, 2836, 6145, 2836), 1, **opts)


@pytest.mark.parametrize("deg", [-44.5, 120.0])
def test_a_turned_stream_comes_back(pkg, torch_cuda, deg):
    """Clean chips at a known angle: the handle's phase and coherence, as the host formats them."""
    torch = torch_cuda
    n, nch = 2836, 3
    xi, xq, _ = cm.rotated(7, 6 * n, deg, sigma_q=40)
    car = pkg.RdsCarrier(nch)
    m = cm.Channel()
    for b in range(6):
        ri, rq = xi[b * n:(b + 1) * n], xq[b * n:(b + 1) * n]
        out = car.feed(torch.from_numpy(np.stack([ri] * nch)).cuda(), torch.from_numpy(np.stack([rq] * nch)).cuda())
        want = m.call(ri, rq)
        assert np.array_equal(out.cpu().numpy()[:, :n], np.stack([want] * nch))
    st = car.stats()
    phase, coh = pkg.rds_carrier_phase_deg(st), pkg.rds_carrier_coherence(st)
    assert np.all(np.abs((phase - deg + 90) % 180 - 90) < 1.0) and np.all(coh > 0.95), (phase, coh)
    assert phase[0] == m.phase_deg() and coh[0] == pytest.approx(m.coherence(), rel=1e-12)
    car.close()


def test_non_finite_samples(pkg, torch_cuda):
    """NaN and +-inf at sample 0, at n - 1 and in the vector tail (n = 2839: the last three samples), in I only, in
    Q only, in a call of several chunks, on several channels beside clean ones that must not change."""
    nan, inf = float("nan"), float("inf")
    sizes = (2839, 2839, 2839, 6145, 2839, 1, 2839)
    poison = {1: [(0, 0, 0, nan), (2, 1, -1, inf), (4, 0, -2, -inf)],       # sample 0 of I; n - 1 of Q; the tail of I
              2: [(1, 1, 0, -inf), (2, 1, 2836, nan), (5, 0, 1000, inf), (5, 1, 1000, nan)],
              3: [(0, 1, 6144, nan), (4, 0, 3072, inf)],                      # the second and third chunk
              5: [(2, 0, 0, nan)]}                                            # a call of one sample
    for shift in (0, 1):
        models = _run_calls(torch_cuda, pkg, 7, sizes, shift, stride_pad=1, poison=poison)
        assert [m.resets for m in models] == [2, 1, 3, 0, 2, 1, 0]
        assert models[3].windows == sum(sizes) // W and models[6].windows == sum(sizes) // W


def test_eight_calls_queued_without_a_host_synchronisation(pkg, torch_cuda):
    torch = torch_cuda
    nch, n, calls = 6, 2836, 8
    xi, xq = _streams(nch, n * calls)
    d_i = torch.from_numpy(xi).cuda()
    d_q = torch.from_numpy(xq).cuda()
    outs = torch.zeros(calls, nch, n, dtype=torch.float32, device="cuda")
    car = pkg.RdsCarrier(nch)
    torch.cuda.synchronize()
    for b in range(calls):                             # views into the streams: rows 8 n floats apart
        car.feed(d_i[:, b * n:(b + 1) * n], d_q[:, b * n:(b + 1) * n], out=outs[b])
    got = outs.cpu().numpy()
    stats = car.stats()
    for c in range(nch):
        m = cm.Channel()
        for b in range(calls):
            want = m.call(xi[c, b * n:(b + 1) * n], xq[c, b * n:(b + 1) * n])
            assert np.array_equal(got[b, c].view(np.uint32), want.view(np.uint32)), (b, c)
        assert _stats_row(stats[c]) == m.stats()
    # reset(): everything, the counters included; the same stream again gives the same rows
    car.reset()
    assert all(_stats_row(r) == cm.Channel().stats() for r in car.stats())
    again = car.feed(d_i[:, :n], d_q[:, :n])
    assert np.array_equal(again.cpu().numpy()[:, :n].view(np.uint32), got[0].view(np.uint32))
    car.close()
