"""GPU: the RDS group decoder (include/sdr_amd.h: sdr_rds_groups and the kernel of sdr_rds.hip) against the
bit-serial model of tests/rds_model.py. Everything is integer and compared exactly: the group records, the
per-call counts, the counters and `synced` after every call, for any cut of the streams into calls."""
from __future__ import annotations

import json

import numpy as np
import pytest

import rds_model as rm
from conftest import GOLD, channel_input

pytestmark = pytest.mark.gpu

NCH = 8
SIZES = (0, 1, 25, 26, 27, 36, 37, 255, 256)
STAT_NAMES = rm.COUNTERS + ("synced",)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def streams(synth):
    return rm.make_streams(synth)


def _plan(streams, seed):
    """The calls [(nbits[NCH], rows[NCH][256])]: sizes from SIZES drawn per channel and call; channel 7 also
    gets -1 and -2 calls; a stream's last call takes what is left."""
    rs = np.random.Generator(np.random.PCG64(seed))
    at = [0] * NCH
    calls = []
    while any(at[c] < len(streams[c]) for c in range(NCH)):
        nb = np.zeros(NCH, np.int32)
        rows = rs.integers(0, 2, (NCH, 256)).astype(np.uint8)       # what lies behind nbits is never read
        for c in range(NCH):
            n = int(rs.choice(SIZES))
            if c == 7 and rs.integers(0, 6) == 0:
                n = int(rs.choice((-1, -1, -2)))
            if n > 0:
                n = min(n, len(streams[c]) - at[c])
                rows[c, :n] = streams[c][at[c]:at[c] + n]
                at[c] += n
            nb[c] = n
        calls.append((nb, rows))
    return calls


def _fixed_plan(streams, size):
    """Every channel `size` bits per call until its stream ends (then 0)."""
    calls, at = [], 0
    longest = max(len(s) for s in streams)
    while at < longest:
        nb = np.zeros(NCH, np.int32)
        rows = np.zeros((NCH, 256), np.uint8)
        for c in range(NCH):
            n = max(0, min(size, len(streams[c]) - at))
            rows[c, :n] = streams[c][at:at + n]
            nb[c] = n
        calls.append((nb, rows))
        at += size
    return calls


def _run_gpu(pkg, torch, calls, check=None, **opts):
    """Feeds the calls; returns (groups per channel, final stats). check(k, groups, counts, stats) after
    every call when given."""
    dec = pkg.RdsDecoder(NCH, **opts)
    got = [[] for _ in range(NCH)]
    d_bits = torch.zeros(NCH, 256, dtype=torch.uint8, device="cuda")
    d_nb = torch.zeros(NCH, dtype=torch.int32, device="cuda")
    for k, (nb, rows) in enumerate(calls):
        d_nb.copy_(torch.from_numpy(nb))
        d_bits.copy_(torch.from_numpy(rows))
        dec.feed(d_nb, d_bits)
        g, n = dec.groups()
        for c in range(NCH):
            got[c] += [g[c, j].tobytes() for j in range(n[c])]
        if check is not None:
            check(k, g, n, dec.stats())
    st = dec.stats()
    dec.close()
    return got, st


def _run_model(calls, **opts):
    chans = [rm.Channel(**opts) for _ in range(NCH)]
    per_call = []
    for nb, rows in calls:
        per_call.append(([ch.call(int(nb[c]), rows[c]) for c, ch in enumerate(chans)],
                         [ch.stats() for ch in chans]))
    return chans, per_call


@pytest.mark.parametrize("max_burst", [0, 2, 5])
def test_parity_with_the_model_after_every_call(pkg, torch_cuda, streams, max_burst):
    calls = _plan(streams, 17 + max_burst)
    assert {int(v) for nb, _ in calls for v in nb} >= set(SIZES) | {-1, -2}
    chans, per_call = _run_model(calls, max_burst=max_burst)

    def check(k, g, n, st):
        want_groups, want_stats = per_call[k]
        for c in range(NCH):
            want = rm.records(want_groups[c])
            assert n[c] == len(want), f"call {k} ch {c}: {n[c]} groups, model {len(want)}"
            assert g[c, :n[c]].tobytes() == want.tobytes(), f"call {k} ch {c}: {g[c, :n[c]]} != {want}"
            for name in STAT_NAMES:
                assert int(st[c][name]) == want_stats[c][name], f"call {k} ch {c} {name}: {st[c]} != {want_stats[c]}"

    _run_gpu(pkg, torch_cuda, calls, check, max_burst=max_burst)
    # the streams do what they were built for
    s = [ch.stats() for ch in chans]
    assert s[0]["bad"] == 0 and s[0]["slips"] == 0 and s[0]["acquired"] == 1 and s[0]["groups"] >= 27
    assert s[2]["slips"] >= 4 and s[4]["lost"] >= 1 and s[4]["acquired"] >= 2
    assert s[6]["groups"] == 0 and s[6]["synced"] == 0 and s[7]["lost"] >= 1
    if max_burst == 5:
        assert s[3]["corrected"] >= 15 and s[3]["bad"] == 0
    if max_burst == 0:
        assert s[3]["corrected"] == 0 and s[3]["bad"] >= 15


def test_split_invariance_on_the_device(pkg, torch_cuda, streams):
    streams = [s[:1500] for s in streams]                    # 1500 one-bit calls
    one, st_one = _run_gpu(pkg, torch_cuda, _fixed_plan(streams, 1))
    big, st_big = _run_gpu(pkg, torch_cuda, _fixed_plan(streams, 256))
    want = [rm.decode(s) for s in streams]
    for c in range(NCH):
        model = [r.tobytes() for r in rm.records(want[c][0])]
        assert one[c] == model, f"ch {c}: one bit per call"
        assert big[c] == model, f"ch {c}: 256 bits per call"
        assert st_one[c].tobytes() == st_big[c].tobytes(), f"ch {c}: {st_one[c]} != {st_big[c]}"
        for name in STAT_NAMES:
            assert int(st_one[c][name]) == want[c][1].stats()[name], (c, name)


def test_sync_switch_inside_one_call(pkg, torch_cuda, synth):
    """With loss_blocks = 2 one 256-bit call holds the loss of sync and the re-acquisition."""
    blocks = []
    for k in range(12):
        blocks += synth.rds_group_0a(0x3000, 3, k & 3, "SWITCH 0")
    bits = rm.blocks_to_bits(blocks)
    rs = np.random.Generator(np.random.PCG64(3))
    stream = bits[:312] + [int(v) for v in rs.integers(0, 2, 60)] + bits[312:]      # 60 = 2 * 26 + 8: out of phase
    cuts = [0, 200, 456, 712, 968, 1224, len(stream)]
    calls = []
    for a, b in zip(cuts, cuts[1:]):
        nb = np.full(NCH, b - a, np.int32)
        rows = np.zeros((NCH, 256), np.uint8)
        rows[:, :b - a] = stream[a:b]
        calls.append((nb, rows))
    chans, per_call = _run_model(calls, loss_blocks=2)
    before, after = per_call[0][1][0], per_call[1][1][0]
    assert (before["synced"], before["lost"], before["acquired"]) == (1, 0, 1)
    assert (after["synced"], after["lost"], after["acquired"]) == (1, 1, 2), after

    def check(k, g, n, st):
        for c in range(NCH):
            want = rm.records(per_call[k][0][c])
            assert g[c, :n[c]].tobytes() == want.tobytes() and n[c] == len(want), (k, c)
            for name in STAT_NAMES:
                assert int(st[c][name]) == per_call[k][1][c][name], (k, c, name)

    _run_gpu(pkg, torch_cuda, calls, check, loss_blocks=2)


def test_refusals(pkg, torch_cuda):
    torch = torch_cuda
    for bad in (dict(max_burst=6), dict(max_burst=-1), dict(loss_blocks=0), dict(loss_blocks=65)):
        with pytest.raises(pkg.SdrError):
            pkg.RdsDecoder(2, **bad)
    with pytest.raises(pkg.SdrError):
        pkg.RdsDecoder(0)
    dec = pkg.RdsDecoder(2)
    nb = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        dec.feed(nb, torch.zeros(2, 255, dtype=torch.uint8, device="cuda"))
    L = pkg.lib()
    assert L.sdr_rds_groups(dec._h, nb.data_ptr(), torch.zeros(2, 256, dtype=torch.uint8, device="cuda").data_ptr(), 255, None) == -1
    assert L.sdr_rds_groups(dec._h, None, None, 256, None) == -1
    dec.close()


def test_pipeline_end_to_end(pkg, torch_cuda, synth):
    """synth channels 0..3, 24 blocks, through Pipeline with feed_pipeline after every block."""
    torch = torch_cuda
    nch, nblocks = 4, 24
    iq = np.stack([channel_input(synth, c, nblocks) for c in range(nch)], axis=1)      # [block][ch][bytes]
    d_iq = torch.from_numpy(iq).cuda()
    pipe = pkg.Pipeline(nch, mode=0, rds_on=True)
    dec = pkg.RdsDecoder(nch)
    models = [rm.Channel() for _ in range(nch)]
    got = [[] for _ in range(nch)]
    want = [[] for _ in range(nch)]
    for b in range(nblocks):
        pipe.frontend(d_iq[b])
        pipe.rds()
        dec.feed_pipeline(pipe)
        g, n = dec.groups()
        nb, bits = pipe.nbits.cpu().numpy(), pipe.bits.cpu().numpy()
        for c in range(nch):
            want[c] += models[c].call(int(nb[c]), bits[c])
            got[c] += [g[c, j] for j in range(n[c])]
    st = dec.stats()
    fixture = json.loads((GOLD / "rds_groups_mode0.json").read_text())
    for c in range(nch):
        w = rm.records(want[c])
        assert np.array(got[c], rm.GROUP_DTYPE).tobytes() == w.tobytes() if got[c] else len(w) == 0, f"ch {c}"
        for name in STAT_NAMES:
            assert int(st[c][name]) == models[c].stats()[name], (c, name)
        station = pkg.RdsStation()
        station.update(np.array(got[c], pkg.rds_group_dtype()))
        assert station.pi == 0x1000 + c, station.text()
        if str(c) in fixture["channels"]:
            lines = [rm.group_line(c, x) for x in want[c]]
            assert lines == fixture["channels"][str(c)]["groups"], f"ch {c}"
            assert station.ps == f"MI355X{c:02d}", station.text()
            assert f"PI: {0x1000 + c:04X}" in station.text() and f"PS: MI355X{c:02d}" in station.text()
    pipe.close()
    dec.close()
