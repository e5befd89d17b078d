"""GPU: the RDS symbol tracker (include/sdr_amd.h: sdr_rds_track_bits and the kernel of sdr_rds_track.hip)
against the model of tests/rds_track_model.py. After the one quantisation everything is integer and compared
exactly: nbits, the bits and the stats record after every call, for calls of every kind of length."""
from __future__ import annotations

import numpy as np
import pytest

import rds_track_model as tm

pytestmark = pytest.mark.gpu

S, B, ROW = tm.S, tm.B, 2836
SIZES = (0, 1, 77, 78, 79, 1000, ROW, tm.MAX_N)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _stats_row(rec) -> dict:
    return {k: int(rec[k]) for k in tm.STATS}


def _compare(k, nch, models, rows, n, nbits, bits, stats):
    for c in range(nch):
        nb, want = models[c].call(rows[c][:n])
        assert int(nbits[c]) == nb, (k, c, n, int(nbits[c]), nb)
        if nb > 0:
            assert bits[c, :nb].tolist() == want, (k, c, n)
        assert _stats_row(stats[c]) == models[c].stats(), (k, c, n)


def _streams(total: int):
    """Five channels of `total` samples, all exact multiples of 2^-QSHIFT: 0 noisy chips; 1 constant bits
    over the acquisition with the right phase at residue 50, so that acquisition takes 11, the wrong half;
    2 noisy chips (it gets the poisoned call); 3 at full scale, beyond the clamp; 4 with a sample missing
    every 2000."""
    k = np.float32(1 << tm.QSHIFT)
    xs = [tm.noise_rows(11, total)[0]]
    rs = np.random.Generator(np.random.PCG64(12))
    bits = [0] * (tm.A + 4) + [int(v) for v in rs.integers(0, 2, total // B + 3)]
    x1 = tm.chips(bits, 300.0)[(-50) % B:][:total]
    x1[(tm.A + 3) * B:] += rs.integers(-150, 151, total - (tm.A + 3) * B).astype(np.float32)
    xs.append((x1 / k).astype(np.float32))
    xs.append(tm.noise_rows(13, total, 200, 300)[0])
    x3, _ = tm.noise_rows(14, total, 300, 100)
    xs.append((x3 * np.float32(200.0)).astype(np.float32))
    x4, _ = tm.noise_rows(15, total + total // 2000 + 1)
    xs.append(np.delete(x4, np.arange(1, total // 2000 + 1) * 2000 - 1)[:total])
    return np.stack(xs)


def test_twelve_calls_of_every_length(pkg, torch_cuda):
    torch = torch_cuda
    nch = 5
    sizes = (ROW, 79, 0, tm.MAX_N, 1, 77, 1000, 78, tm.MAX_N, ROW, 1000, 77)
    assert len(sizes) == 12 and set(sizes) == set(SIZES)
    poison_call = 6                                   # 1000 samples, an acquisition's worth and more behind it
    x = _streams(sum(sizes))
    models = [tm.Channel() for _ in range(nch)]
    trk = pkg.RdsTracker(nch)
    d_row = torch.zeros(nch, tm.MAX_N, dtype=torch.float32, device="cuda")
    d_bits = torch.full((nch, 256), 7, dtype=torch.uint8, device="cuda")
    d_nb = torch.full((nch,), -9, dtype=torch.int32, device="cuda")
    at = 0
    for k, n in enumerate(sizes):
        rows = x[:, at:at + n].copy()
        at += n
        if k == poison_call:
            rows[2, n // 2] = np.nan
        if n:
            d_row[:, :n].copy_(torch.from_numpy(rows))
        trk.feed(d_row, n, nbits=d_nb, bits=d_bits)
        stats = trk.stats()
        _compare(k, nch, models, rows, n, d_nb.cpu().numpy(), d_bits.cpu().numpy(), stats)
    final = [m.stats() for m in models]
    assert all(s["locked"] == 1 for s in final), final
    assert final[1]["half_moves"] == 1 and final[1]["phase"] == 50          # left the wrong half
    assert final[2]["resets"] == 1 and final[2]["acquired"] == 2            # poisoned once, acquired again
    assert final[3]["level"] == tm.T * B * tm.QMAX                          # the clamp, every sample
    assert final[4]["moves"] >= 10 and final[0]["resets"] == 0
    trk.reset()
    assert all(_stats_row(r) == dict.fromkeys(tm.STATS, 0) for r in trk.stats())
    trk.close()


@pytest.mark.parametrize("nch,shift", [(1, 0), (1, 1), (67, 1)])
def test_alignment_and_stride(pkg, torch_cuda, nch, shift):
    """Rows 2839 floats apart from a base `shift` floats past a 16-byte boundary: with 67 channels a quarter
    of the rows are 16-byte aligned and staged with vector loads, the others with scalar loads."""
    torch = torch_cuda
    stride, calls = ROW + 3, (ROW, ROW, 1000, ROW, 79)
    x = np.stack([tm.noise_rows(100 + c, sum(calls))[0] for c in range(nch)])
    flat = torch.zeros(nch * stride + 8, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    d_row = flat[shift:shift + nch * stride].view(nch, stride)
    aligned = sum(1 for c in range(nch) if (d_row.data_ptr() + 4 * stride * c) % 16 == 0)
    assert aligned == {(1, 0): 1, (1, 1): 0, (67, 1): 17}[(nch, shift)]
    models = [tm.Channel() for _ in range(nch)]
    trk = pkg.RdsTracker(nch)
    at = 0
    for k, n in enumerate(calls):
        rows = x[:, at:at + n]
        at += n
        d_row[:, :n].copy_(torch.from_numpy(np.ascontiguousarray(rows)))
        d_nb, d_bits = trk.feed(d_row, n)
        stats = trk.stats()
        _compare(k, nch, models, rows, n, d_nb.cpu().numpy(), d_bits.cpu().numpy(), stats)
    assert all(m.locked for m in models) and sum(m.bits for m in models) > 60 * nch
    trk.close()
