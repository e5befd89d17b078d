"""GPU: the RDS soft decisions (include/sdr_amd.h: sdr_rds_track_bits_soft, sdr_rds_groups_soft and the kernels of
sdr_rds_track.hip and sdr_rds.hip) against the model of tests/rds_soft_model.py. Everything is integer and
compared exactly after every call: the tracker's soft rows beside its bits, the decoder's group records with
their flags, its counters and its soft counters, for any cut of the streams into calls."""
from __future__ import annotations

import numpy as np
import pytest

import rds_model as rm
import rds_soft_model as sm
import rds_track_model as tm

pytestmark = pytest.mark.gpu

ROW = 2836
STAT_NAMES = rm.COUNTERS + ("synced",)
SENTINEL = 0x7777


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _u16(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint16)


# ------------------------------------------------------------------ the tracker
def _track_streams(total: int) -> np.ndarray:
    """Four channels: noisy chips; weak chips under +-2500 of noise; noisy chips (it gets the poisoned call);
    full scale, beyond the clamp (soft = SOFT_MAX)."""
    rs = np.random.Generator(np.random.PCG64(31))
    bits = [int(v) for v in rs.integers(0, 2, total // tm.B + 2)]
    x3 = (tm.noise_rows(34, total, 300, 100)[0] * np.float32(200.0)).astype(np.float32)
    return np.stack([tm.noise_rows(32, total)[0], sm.noisy_chips(bits, 33)[:total], tm.noise_rows(35, total, 200, 300)[0], x3])


@pytest.mark.parametrize("shift", [0, 1])
def test_tracker_soft_rows_of_every_call_length(pkg, torch_cuda, shift):
    """Rows on 16-byte boundaries (shift 0: vector loads) and one float off (scalar loads); the soft rows are 256
    wide with a guard row on either side, and a second handle runs sdr_rds_track_bits on the same calls."""
    torch = torch_cuda
    nch = 4
    sizes = (ROW, 79, 0, tm.MAX_N, 1, 77, 1000, 78, 3073, ROW, 1000)
    poison_call = 6
    x = _track_streams(sum(sizes))
    models = [sm.TrackChannel() for _ in range(nch)]
    trk, hard = pkg.RdsTracker(nch), pkg.RdsTracker(nch)
    stride = tm.MAX_N + 4
    flat = torch.zeros(nch * stride + 8, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    d_row = flat[shift:shift + nch * stride].view(nch, stride)
    guarded = torch.full((nch + 2, 256), SENTINEL, dtype=torch.int16, device="cuda")
    d_soft = guarded[1:nch + 1]
    at = 0
    for k, n in enumerate(sizes):
        rows = x[:, at:at + n].copy()
        at += n
        if k == poison_call:
            rows[2, n // 2] = np.inf
        if n:
            d_row[:, :n].copy_(torch.from_numpy(rows))
        guarded.fill_(SENTINEL)
        d_nb, d_bits, got_soft = trk.feed(d_row, n, soft=d_soft)
        assert got_soft is d_soft
        h_nb, h_bits = hard.feed(d_row, n)
        nb, bits, soft, all_soft = d_nb.cpu().numpy(), d_bits.cpu().numpy(), _u16(d_soft), _u16(guarded)
        assert np.array_equal(nb, h_nb.cpu().numpy()), k
        stats = trk.stats()
        assert stats.tobytes() == hard.stats().tobytes(), k
        assert (all_soft[0] == SENTINEL).all() and (all_soft[-1] == SENTINEL).all(), f"call {k}: a guard row was written"
        for c in range(nch):
            want_nb, want_bits, want_soft = models[c].call(rows[c][:n])
            assert int(nb[c]) == want_nb, (k, c, n)
            m = max(want_nb, 0)
            assert bits[c, :m].tolist() == want_bits and h_bits[c, :m].cpu().tolist() == want_bits, (k, c, n)
            assert soft[c, :m].tolist() == want_soft, (k, c, n)
            assert (soft[c, m:] == SENTINEL).all(), f"call {k} ch {c}: soft values behind nbits = {want_nb}"
            assert {name: int(stats[c][name]) for name in tm.STATS} == models[c].stats(), (k, c)
    assert all(m.locked for m in models) and models[2].resets == 1
    assert models[3].level == tm.T * tm.B * tm.QMAX
    # own tensor, allocated on first use
    assert trk.soft is None
    out = trk.feed(d_row, 0, soft=True)
    assert len(out) == 3 and out[2] is trk.soft and tuple(trk.soft.shape) == (nch, 256) and trk.soft.element_size() == 2
    trk.close()
    hard.close()


# ------------------------------------------------------------------ the decoder
@pytest.fixture(scope="module")
def channels(synth):
    """(bits, softs) per channel: the eight soft streams (channel 7 gets the -1 and -2 calls), then the model
    file's hand-built cases."""
    streams, softs = sm.make_soft_streams(synth)
    clean = rm.make_streams(synth)[0]
    cases = sm.hand_built_cases(clean)
    return [s[:1560] for s in streams] + [c[1] for c in cases], [v[:1560] for v in softs] + [c[2] for c in cases]


def _plan(channels, sizes, seed, idle_channel=None):
    """The calls [(nbits[nch], bits[nch][256], soft[nch][256])]: per call and channel a size drawn from `sizes`;
    idle_channel also gets -1, -2 and out-of-range calls. What lies behind nbits is random and never read."""
    bits, softs = channels
    nch = len(bits)
    rs = np.random.Generator(np.random.PCG64(seed))
    at = [0] * nch
    calls = []
    while any(at[c] < len(bits[c]) for c in range(nch)):
        nb = np.zeros(nch, np.int32)
        rows = rs.integers(0, 2, (nch, 256)).astype(np.uint8)
        srow = rs.integers(0, 65536, (nch, 256)).astype(np.uint16)
        for c in range(nch):
            n = int(rs.choice(sizes))
            if c == idle_channel and len(calls) % 4 == 3:     # every fourth call, each kind in turn
                n = (-1, -2, 257, -3)[(len(calls) // 4) % 4]
            if n > 0 and n <= 256:
                n = min(n, len(bits[c]) - at[c])
                rows[c, :n] = bits[c][at[c]:at[c] + n]
                srow[c, :n] = softs[c][at[c]:at[c] + n]
                at[c] += n
            nb[c] = n
        calls.append((nb, rows, srow))
    return calls


def _check_decoder(pkg, torch, calls, nch, every=1, **opts):
    """Feeds the calls to a soft decoder and to the models; groups are compared after every call, the counters
    after every `every`-th and the last. Returns the models."""
    models = [sm.Channel(**opts) for _ in range(nch)]
    dec = pkg.RdsDecoder(nch, soft=True, **opts)
    d_nb = torch.zeros(nch, dtype=torch.int32, device="cuda")
    d_bits = torch.zeros(nch, 256, dtype=torch.uint8, device="cuda")
    d_soft = torch.zeros(nch, 256, dtype=torch.int16, device="cuda")
    for k, (nb, rows, srow) in enumerate(calls):
        d_nb.copy_(torch.from_numpy(nb))
        d_bits.copy_(torch.from_numpy(rows))
        d_soft.copy_(torch.from_numpy(srow.view(np.int16)))
        dec.feed(d_nb, d_bits, soft=d_soft)
        g, n = dec.groups()
        for c in range(nch):
            want = rm.records(models[c].call(int(nb[c]), rows[c], srow[c]))
            assert n[c] == len(want), f"call {k} ch {c}: {n[c]} groups, model {len(want)}"
            assert g[c, :n[c]].tobytes() == want.tobytes(), f"call {k} ch {c}: {g[c, :n[c]]} != {want}"
        if k % every == 0 or k == len(calls) - 1:
            st, ss = dec.stats(), dec.soft_stats()
            for c in range(nch):
                for name in STAT_NAMES:
                    assert int(st[c][name]) == models[c].stats()[name], f"call {k} ch {c} {name}: {st[c]} != {models[c].stats()}"
                assert {f: int(ss[c][f]) for f in ss.dtype.names} == models[c].soft_stats(), f"call {k} ch {c}: {ss[c]}"
    dec.close()
    return models


@pytest.mark.parametrize("L", [0, 1, 4, 6])
@pytest.mark.parametrize("cut", ["1", "36/37", "256", "random"])
def test_decoder_parity_with_the_model(pkg, torch_cuda, channels, L, cut):
    nch = len(channels[0])
    if cut == "1":                                             # every judgement's window lies in the history
        chans = ([b[:700] for b in channels[0]], [v[:700] for v in channels[1]])
        calls, every = _plan(chans, (1,), 1), 64
    else:
        sizes = {"36/37": (36, 37), "256": (256,), "random": (0, 1, 25, 26, 27, 28, 36, 37, 100, 255, 256)}[cut]
        calls, every = _plan(channels, sizes, 2 + L, idle_channel=7 if cut == "random" else None), 1
    if cut == "random":
        assert {int(v) for nb, _, _ in calls for v in nb} >= {0, 1, 256, -1, -2, 257}
    models = _check_decoder(pkg, torch_cuda, calls, nch, every, soft_bits=L)
    s = [m.soft_stats() for m in models]
    if L == 0:
        assert all(v["soft_blocks"] == 0 for v in s)
    else:
        assert s[0]["soft_blocks"] >= 1 and s[8 + 5]["soft_blocks"] >= 1, s[:14]        # stream 0; "raw 5"
    if L == 6 and cut != "1":
        assert sum(v["soft_flips"] for v in s[:8]) > sum(v["soft_blocks"] for v in s[:8])


def test_257_channels_through_a_reset(pkg, torch_cuda, channels):
    torch = torch_cuda
    nch = 257
    bits = [channels[0][c % 8][26 * (c // 8):][:700] for c in range(nch)]
    softs = [channels[1][c % 8][26 * (c // 8):][:700] for c in range(nch)]
    calls = _plan((bits, softs), (256,), 9)
    models = [sm.Channel(soft_bits=6) for _ in range(nch)]
    dec = pkg.RdsDecoder(nch, soft_bits=6)
    d_nb = torch.zeros(nch, dtype=torch.int32, device="cuda")
    d_bits = torch.zeros(nch, 256, dtype=torch.uint8, device="cuda")
    d_soft = torch.zeros(nch, 256, dtype=torch.int16, device="cuda")
    for rnd in range(2):
        for k, (nb, rows, srow) in enumerate(calls):
            d_nb.copy_(torch.from_numpy(nb))
            d_bits.copy_(torch.from_numpy(rows))
            d_soft.copy_(torch.from_numpy(srow.view(np.int16)))
            dec.feed(d_nb, d_bits, soft=d_soft)
            g, n = dec.groups()
            for c in range(nch):
                want = rm.records(models[c].call(int(nb[c]), rows[c], srow[c]))
                assert n[c] == len(want) and g[c, :n[c]].tobytes() == want.tobytes(), (rnd, k, c)
        st, ss = dec.stats(), dec.soft_stats()
        for c in range(nch):
            assert {name: int(st[c][name]) for name in STAT_NAMES} == models[c].stats(), (rnd, c)
            assert {f: int(ss[c][f]) for f in ss.dtype.names} == models[c].soft_stats(), (rnd, c)
        assert sum(m.soft_blocks for m in models) > nch
        dec.reset()
        for m in models:
            m.reset()
        st, ss = dec.stats(), dec.soft_stats()
        assert not st.view(np.uint32).any() and not ss["soft_blocks"].any() and not ss["soft_flips"].any()
        assert (ss["soft_bits"] == 6).all()
    dec.close()


def test_the_two_kinds_of_handle_refuse_each_other(pkg, torch_cuda):
    torch = torch_cuda
    nb = torch.zeros(2, dtype=torch.int32, device="cuda")
    bits = torch.zeros(2, 256, dtype=torch.uint8, device="cuda")
    soft = torch.zeros(2, 256, dtype=torch.int16, device="cuda")
    hard, softd, soft0 = pkg.RdsDecoder(2), pkg.RdsDecoder(2, soft_bits=3), pkg.RdsDecoder(2, soft=True)
    assert (hard.soft, softd.soft, soft0.soft) == (False, True, True)
    with pytest.raises(pkg.SdrError):
        hard.feed(nb, bits, soft=soft)
    for d in (softd, soft0):
        with pytest.raises(pkg.SdrError):
            d.feed(nb, bits)
        d.feed(nb, bits, soft=soft)
    hard.feed(nb, bits)
    assert [int(v) for v in softd.soft_stats()["soft_bits"]] == [3, 3] and not hard.soft_stats().view(np.uint32).any()
    L = pkg.lib()
    assert L.sdr_rds_groups_soft(softd._h, nb.data_ptr(), bits.data_ptr(), 256, soft.data_ptr(), 255, None) == -1
    assert L.sdr_rds_groups_soft(softd._h, nb.data_ptr(), bits.data_ptr(), 256, None, 256, None) == -1
    with pytest.raises(ValueError):
        softd.feed(nb, bits, soft=torch.zeros(2, 255, dtype=torch.int16, device="cuda"))
    for bad in (dict(soft_bits=7), dict(soft_bits=-1), dict(soft_bits=2, max_burst=6), dict(soft_bits=2, loss_blocks=0)):
        with pytest.raises(pkg.SdrError):
            pkg.RdsDecoder(2, **bad)
    for d in (hard, softd, soft0):
        d.close()


def test_end_to_end_on_the_device(pkg, torch_cuda, synth):
    """The clean stream at amplitude 300 under +-2500 of noise (seeds 1 and 2, one channel each) through the soft
    tracker into the soft decoder and, the same bits, into the hard decoder: equal to the models call by call,
    and more complete groups with the soft step than without."""
    torch = torch_cuda
    clean = rm.make_streams(synth)[0]
    x = np.stack([sm.noisy_chips(clean, seed) for seed in (1, 2)])
    nch = 2
    trk, soft_dec, hard_dec = pkg.RdsTracker(nch), pkg.RdsDecoder(nch, soft_bits=6), pkg.RdsDecoder(nch)
    tmod = [sm.TrackChannel() for _ in range(nch)]
    smod, hmod = [sm.Channel(soft_bits=6) for _ in range(nch)], [rm.Channel() for _ in range(nch)]
    got = {"soft": [[] for _ in range(nch)], "hard": [[] for _ in range(nch)]}
    want = {"soft": [[] for _ in range(nch)], "hard": [[] for _ in range(nch)]}
    d_row = torch.zeros(nch, ROW, dtype=torch.float32, device="cuda")
    for at in range(0, x.shape[1], ROW):
        rows = x[:, at:at + ROW]
        n = rows.shape[1]
        d_row[:, :n].copy_(torch.from_numpy(np.ascontiguousarray(rows)))
        d_nb, d_bits, d_soft = trk.feed(d_row, n, soft=True)
        soft_dec.feed(d_nb, d_bits, soft=d_soft)
        hard_dec.feed(d_nb, d_bits)
        nb, bits, soft = d_nb.cpu().numpy(), d_bits.cpu().numpy(), _u16(d_soft)
        for name, dec in (("soft", soft_dec), ("hard", hard_dec)):
            g, cnt = dec.groups()
            for c in range(nch):
                got[name][c] += [g[c, j].tobytes() for j in range(cnt[c])]
        for c in range(nch):
            want_nb, want_bits, want_soft = tmod[c].call(rows[c])
            assert int(nb[c]) == want_nb and bits[c, :want_nb].tolist() == want_bits and soft[c, :want_nb].tolist() == want_soft, (at, c)
            want["soft"][c] += smod[c].call(want_nb, want_bits, want_soft)
            want["hard"][c] += hmod[c].call(want_nb, want_bits)
    ss = soft_dec.soft_stats()
    for c in range(nch):
        for name in ("soft", "hard"):
            assert got[name][c] == [r.tobytes() for r in rm.records(want[name][c])], (name, c)
        full = {name: sum(1 for g in want[name][c] if g[1] == 15) for name in ("soft", "hard")}
        print(f"seed {c + 1}: complete groups hard {full['hard']} soft {full['soft']}; {smod[c].stats()} {smod[c].soft_stats()}")
        assert full["soft"] > full["hard"] and smod[c].bad < hmod[c].bad
        assert int(ss[c]["soft_blocks"]) == smod[c].soft_blocks >= 20 and int(ss[c]["soft_flips"]) == smod[c].soft_flips
    for h in (trk, soft_dec, hard_dec):
        h.close()
