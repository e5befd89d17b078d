"""GPU: the life of the seven stage handles (Scanner, Splitter, Meter, AudioFinish, RdsDecoder, RdsTracker,
RdsCarrier) at 1, 256 and 257 channels (capture rows, wide streams): the bounds of the one-thread-per-channel
grid of the reset and stats kernels, 257 being the first size with a second workgroup. For each: the records of
a fresh handle, one real call on a tiny input after which the records are what the definition says (and not the
fresh ones), reset() after which they are the fresh handle's byte for byte -- the last channel's among them --
and close() twice, the second a no-op. The kernels' results have their own tests against the models; this one
is about create, reset, the record reads and destroy (csrc/stage_host.h).

RdsTracker at 257 is tests/test_gpu_rds_track_edges.py::test_reset_with_a_second_block_of_channels and is not
repeated here."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import rds_model as rm
import rds_soft_model as sm

pytestmark = pytest.mark.gpu

SIZES = (1, 256, 257)
N_TINY = 78 * 4                     # four bits of the tracker's clock: far less than a window of the derotator


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _closed_twice(h):
    h.close()
    assert h._h is None
    h.close()                       # nothing left to destroy: a second sdr_*_destroy of the handle would be a double free
    assert h._h is None


def _bytes(*arrays) -> bytes:
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


@pytest.mark.parametrize("nsrc", SIZES)
def test_scanner(pkg, torch_cuda, nsrc):
    torch = torch_cuda
    sc = pkg.Scanner(3, nsrc)       # mode 3: the shortest block
    fresh = sc.psd()
    assert not fresh[0].any() and fresh[1] == 0
    iq = torch.randint(0, 256, (nsrc, 2 * sc.block_iq), dtype=torch.uint8, device="cuda",
                       generator=torch.Generator("cuda").manual_seed(1))
    sc.block(iq)
    psd, seg = sc.psd()
    assert seg == sc.segments_per_block and (psd.sum(axis=1) > 0).all()      # every row has power, the last one too
    sc.reset()
    again = sc.psd()
    assert _bytes(again[0]) == _bytes(fresh[0]) and again[1] == 0
    _closed_twice(sc)


@pytest.mark.parametrize("nwide", SIZES)
def test_splitter(pkg, torch_cuda, nwide):
    """The history is not among the records: the rows of the same block after reset() are those of the fresh
    handle, which they are not without it. Shift 1 keeps a bit of every sum, so full-range noise clips in every
    row (an output byte holds |sum| < 256 only)."""
    torch = torch_cuda
    sp = pkg.Splitter(4, nwide, mode=3, shift=1)
    fresh = sp.clips()
    assert fresh.shape == (nwide, 7) and not fresh.any()
    wide = torch.randint(-128, 128, (nwide, 2 * sp.wide_iq), dtype=torch.int8, device="cuda",
                         generator=torch.Generator("cuda").manual_seed(2))
    first = sp.block(wide).clone()
    clips = sp.clips()
    assert (clips > 0).all()
    second = sp.block(wide).clone()                                          # behind a history that is not silence
    assert not torch.equal(first[:, :64], second[:, :64])
    sp.reset()
    assert _bytes(sp.clips()) == _bytes(fresh)
    assert torch.equal(sp.block(wide), first) and np.array_equal(sp.clips(), clips)
    _closed_twice(sp)


@pytest.mark.parametrize("nch", SIZES)
def test_meter_and_audio_finish(pkg, torch_cuda, nch):
    """One block of one context feeds both: the meter's rows and the finishing stage's state."""
    torch = torch_cuda
    pipe, meter, fin = pkg.Pipeline(nch, rds_on=False), pkg.Meter(nch), pkg.AudioFinish(nch)
    rows0, state0 = meter.rows(), fin.state()
    assert _bytes(rows0) == bytes(64 * nch)
    assert all((state0[k] == v).all() for k, v in (("y", 0.0), ("blend", 1.0), ("gain", 1.0), ("blend_target", 1.0),
                                                    ("gain_target", 1.0)))
    iq = torch.randint(0, 256, (nch, 2 * pipe.info.block_iq), dtype=torch.uint8, device="cuda",
                       generator=torch.Generator("cuda").manual_seed(3))
    pipe.frontend(iq)
    lr = pipe.stereo()
    meter.audio(pipe, lr)
    fin.set_control(blend=0.25, gain=0.5)
    fin.finish(lr)
    rows, state = meter.rows(), fin.state()
    assert (rows["fm_sq"] > 0).all() and (rows["flags"] != 0).all()          # noise has power in every channel
    assert (state["blend_target"] == 0.25).all() and (state["gain_target"] == 0.5).all()
    assert (state["blend"] == 0.25).all() and (state["gain"] == 0.5).all()   # reached by the end of the block's ramp
    meter.reset()
    fin.reset()
    assert _bytes(meter.rows()) == _bytes(rows0) and _bytes(fin.state()) == _bytes(state0)
    for h in (meter, fin, pipe):
        _closed_twice(h)


@pytest.mark.parametrize("nch", SIZES)
def test_rds_decoder(pkg, torch_cuda, synth, nch):
    """A soft handle, for both of its record reads; every channel gets the first 256 bits of the same clean
    stream, which the model synchronises on."""
    torch = torch_cuda
    bits = np.asarray(rm.make_streams(synth)[0][:256], np.uint8)
    model = sm.Channel()
    model.call(256, bits, np.zeros(256, np.uint16))
    want = model.stats()
    assert want["acquired"] == 1 and want["groups"] >= 1 and want["synced"] == 1
    dec = pkg.RdsDecoder(nch, soft_bits=6)
    fresh = (dec.stats(), dec.soft_stats(), *dec.groups())
    assert not fresh[0].view(np.uint32).any() and (fresh[1]["soft_bits"] == 6).all() and not fresh[3].any()
    d_nb = torch.full((nch,), 256, dtype=torch.int32, device="cuda")
    d_bits = torch.from_numpy(bits).cuda().repeat(nch, 1)
    d_soft = torch.zeros(nch, 256, dtype=torch.int16, device="cuda")
    dec.feed(d_nb, d_bits, soft=d_soft)
    st, (g, n) = dec.stats(), dec.groups()
    for name in rm.COUNTERS + ("synced",):
        assert (st[name] == want[name]).all(), name
    assert (n >= 1).all()
    dec.reset()
    assert _bytes(dec.stats(), dec.soft_stats(), *dec.groups()) == _bytes(*fresh)
    _closed_twice(dec)


def _tiny_rows(torch, nch, seed):
    """[nch][N_TINY] finite rows, and the same with a NaN in every channel: such a call uses none of its samples and
    counts one reset per channel (include/sdr_amd.h), which is what a call this short can count"""
    x = torch.randn(nch, N_TINY, dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))
    bad = x.clone()
    bad[:, 5] = float("nan")
    return x, bad


@pytest.mark.parametrize("nch", SIZES[:2])
def test_rds_tracker(pkg, torch_cuda, nch):
    torch = torch_cuda
    trk = pkg.RdsTracker(nch)
    fresh = trk.stats()
    assert not fresh.view(np.uint32).any()
    x, bad = _tiny_rows(torch, nch, 4)
    nb, _ = trk.feed(x)
    assert (nb.cpu().numpy() >= 0).all()
    nb, _ = trk.feed(bad)
    st = trk.stats()
    assert (nb.cpu().numpy() == pkg.SDR_NBITS_POISONED).all() and (st["resets"] == 1).all()
    trk.reset()
    assert _bytes(trk.stats()) == _bytes(fresh)
    _closed_twice(trk)


@pytest.mark.parametrize("nch", SIZES)
def test_rds_carrier(pkg, torch_cuda, nch):
    torch = torch_cuda
    car = pkg.RdsCarrier(nch)
    fresh = car.stats()
    assert not fresh.view(np.uint8).any()
    (xi, bad), (xq, _) = _tiny_rows(torch, nch, 5), _tiny_rows(torch, nch, 6)
    out = car.feed(xi, xq)
    assert torch.isfinite(out[:, :N_TINY]).all()
    assert _bytes(car.stats()) == _bytes(fresh)                              # no window has ended: nothing counted yet
    out = car.feed(bad, xq)
    st = car.stats()
    assert torch.isnan(out[:, :N_TINY]).all() and (st["resets"] == 1).all() and (st["windows"] == 0).all()
    car.reset()
    assert _bytes(car.stats()) == _bytes(fresh)
    _closed_twice(car)


def test_tuner_set_says_what_the_check_says(pkg, torch_cuda):
    """sdr_tuner_set on a context against sdr_tuner_check (tests/test_opts_check.py holds the check against the
    documented rule): the same verdict, and the same text behind the name."""
    L = pkg.lib()
    nch = 3
    pipe = pkg.Pipeline(nch)
    arr = lambda v: (C.c_int32 * nch)(*v)
    for nsrc, src, khz in ((-1, (0, 0, 0), (0, 0, 0)), (4, (0, 0, 0), (0, 0, 0)), (2, (0, 2, 1), (0, 0, 0)),
                           (1, (0, 0, -1), (0, 0, 0)), (1, (0, 0, 0), (0, 0, -1200)), (1, (0, 0, 0), (1201, 0, 0)),
                           (2, (0, 1, 1), (1200, -1199, 7)), (1, None, (0, 0, 0)), (1, (0, 0, 0), None), (0, None, None)):
        s, k = (arr(src) if src else None), (arr(khz) if khz else None)
        rc = L.sdr_tuner_check(0, nch, nsrc, s, k)
        said = L.sdr_last_error().decode()
        assert L.sdr_tuner_set(pipe._h, nsrc, s, k, None) == rc, (nsrc, src, khz)
        if rc != 0:
            text = L.sdr_last_error().decode()
            assert text.startswith("tuner_set: ") and text.split(": ", 1)[1] == said.split(": ", 1)[1], (text, said)
        else:
            assert pipe.nsrc == nsrc
    _closed_twice(pipe)
