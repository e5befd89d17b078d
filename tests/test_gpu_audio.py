"""GPU: the audio finishing stage (include/sdr_amd.h: sdr_audio_finish, sdr_audio_blend_from_meter, the
kernels of sdr_audio.hip) against the CPU model of tests/audio_model.py. Every comparison is bit for
bit: the int16 rows, and every float of the state as uint32."""
from __future__ import annotations

import numpy as np
import pytest

import audio_model as am
import meter_model as mm
from conftest import channel_input

pytestmark = pytest.mark.gpu

N = am.N_AUDIO
NB_KINDS = 10


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _assert_state(got, want, what):
    bad = am.same_state(got, want)
    assert not bad, f"{what}: state differs in {bad}\n got  {got}\n want {want}"


def _assert_rows(got, want, what):
    if not np.array_equal(got, want):
        ch, i = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: {int((got != want).sum())} samples differ, first at channel {ch} sample {i}: "
                             f"{got[ch, i]} != {want[ch, i]}")


def _padded(torch, block, stride):
    """block [nch][len] on the device inside rows of `stride` int16, the padding filled with a pattern."""
    buf = torch.full((block.shape[0], stride), 12345, dtype=torch.int16, device="cuda")
    view = buf[:, :block.shape[1]]
    view.copy_(torch.from_numpy(block))
    return buf, view


def _run_random(pkg, torch, nch, seed, in_place=False):
    """3 blocks of random full-range int16, new random blend and gain targets before each block,
    strides 2N+6 in and 2N+10 out (2N+6 both when in place): the GPU's blocks and states and the model's."""
    rs = np.random.Generator(np.random.PCG64(seed))
    fin = pkg.AudioFinish(nch)
    model = am.AudioFinish(nch)
    out = []
    for b in range(3):
        x = rs.integers(-32768, 32768, (nch, 2 * N), dtype=np.int16)
        blend = rs.uniform(0, 1, nch).astype(np.float32)
        gain = rs.uniform(0, 2.5, nch).astype(np.float32)
        if b == 1:
            blend[0], gain[0] = 0.0, 0.0
        fin.set_control(blend, gain)
        model.set_control(blend, gain)
        ibuf, iview = _padded(torch, x, 2 * N + 6)
        if in_place:
            fin.finish(iview, out=iview)
            obuf, oview = ibuf, iview
        else:
            obuf, oview = _padded(torch, np.zeros_like(x), 2 * N + 10)
            fin.finish(iview, out=oview)
        got, state = oview.cpu().numpy(), fin.state()
        want = model.finish(x)
        out.append((got, state, want, model.state()))
        assert (obuf[:, 2 * N:] == 12345).all(), "the padding of the output rows was written"
        if not in_place:
            assert np.array_equal(iview.cpu().numpy(), x), "the input rows were written"
    fin.close()
    return out


@pytest.fixture(scope="module")
def random70(pkg, torch_cuda):
    return _run_random(pkg, torch_cuda, 70, 21)


def test_random_rows_ramps_and_a_partial_group(random70):
    for b, (got, state, want, wstate) in enumerate(random70):
        _assert_rows(got, want, f"block {b}")
        _assert_state(state, wstate, f"block {b}")
    st = random70[1][1]
    assert st["gain"][0] == 0 and st["blend"][0] == 0 and np.array_equal(st["gain"], st["gain_target"])


def test_random_rows_one_channel(pkg, torch_cuda):
    for b, (got, state, want, wstate) in enumerate(_run_random(pkg, torch_cuda, 1, 22)):
        _assert_rows(got, want, f"block {b}")
        _assert_state(state, wstate, f"block {b}")


def test_in_place(pkg, torch_cuda, random70):
    for b, (got, state, _, _) in enumerate(_run_random(pkg, torch_cuda, 70, 21, in_place=True)):
        _assert_rows(got, random70[b][0], f"block {b}")
        _assert_state(state, random70[b][1], f"block {b}")


def test_decay_through_subnormals(pkg, torch_cuda):
    """The impulse row of the model test beside a random neighbour, two blocks: would fail under
    flush-to-zero (the state ends at +-2 denormal steps)."""
    torch = torch_cuda
    rs = np.random.Generator(np.random.PCG64(23))
    x = np.zeros((2, 2 * N), np.int16)
    x[0, 0], x[0, 1] = 32767, -20000
    x[1] = rs.integers(-32768, 32768, 2 * N, dtype=np.int16)
    fin, model = pkg.AudioFinish(2), am.AudioFinish(2)
    for b in range(2):
        blk = x if b == 0 else np.zeros_like(x)
        got = fin.finish(torch.from_numpy(blk).cuda()).cpu().numpy()
        _assert_rows(got, model.finish(blk), f"block {b}")
        _assert_state(fin.state(), model.state(), f"block {b}")
    y = fin.state()["y"][0]
    assert y[0] == np.float32(2.0 ** -148) and y[1] == -np.float32(2.0 ** -148), y
    fin.close()


def test_identity(pkg, torch_cuda):
    torch = torch_cuda
    rs = np.random.Generator(np.random.PCG64(24))
    x = rs.integers(-32768, 32768, (5, 2 * N), dtype=np.int16)
    x[0, :9] = -32768
    fin = pkg.AudioFinish(5, tau_us=0.0)
    for _ in range(2):
        got = fin.finish(torch.from_numpy(x).cuda()).cpu().numpy()
        _assert_rows(got, np.maximum(x, -32767), "identity")
    fin.close()


def test_poison(pkg, torch_cuda):
    """Channel 1 all poison in block 1 of 3; channel 2 carries some -32768 samples (and a first frame of
    them) but is audio."""
    torch = torch_cuda
    rs = np.random.Generator(np.random.PCG64(25))
    x = rs.integers(-32768, 32768, (3, 4, 2 * N), dtype=np.int16)
    x[1, 1] = -32768
    x[1, 2, :200] = -32768
    x[1, 2, 1001] = -32768
    x[1, 3, :-1] = -32768                              # all but the last sample
    fin, model = pkg.AudioFinish(4), am.AudioFinish(4)
    fresh = am.AudioFinish(4)
    for b in range(3):
        got = fin.finish(torch.from_numpy(x[b]).cuda()).cpu().numpy()
        _assert_rows(got, model.finish(x[b]), f"block {b}")
        st = fin.state()
        _assert_state(st, model.state(), f"block {b}")
        if b == 1:
            assert (got[1] == -32768).all() and not st["y"][1].any()
            assert not (got[2] == -32768).any() and not (got[3] == -32768).any() and st["y"][3].all()
        if b == 2:
            assert np.array_equal(got[1], fresh.finish(x[2])[1]), "block 2 is not the model restarted from 0"
    fin.close()


def test_width_1_on_mono_rows(pkg, synth, torch_cuda):
    torch = torch_cuda
    nch, nb = 3, 2
    iq = np.stack([channel_input(synth, c, nb) for c in range(nch)], axis=1)
    pipe = pkg.Pipeline(nch)
    fin, model = pkg.AudioFinish(nch, width=1, tau_us=50.0), am.AudioFinish(nch, width=1, tau_us=50.0)
    fin.set_control(gain=[1.0, 0.5, 2.0])
    model.set_control(gain=[1.0, 0.5, 2.0])
    for b in range(nb):
        pipe.frontend(torch.from_numpy(iq[b]).cuda())
        mono = pipe.mono()
        got = fin.finish(mono).cpu().numpy()
        _assert_rows(got, model.finish(mono.cpu().numpy()), f"block {b}")
        _assert_state(fin.state(), model.state(), f"block {b}")
        assert got.any()
    fin.close()
    pipe.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_other_modes_on_stereo_rows(pkg, synth, torch_cuda, mode):
    torch = torch_cuda
    nch, nb = 3, 2
    info = pkg.Pipeline(1, mode=mode).info
    assert info.n_audio == N
    need = nb * 2 * info.block_iq
    rows = []
    for c in range(nch):
        have = channel_input(synth, c, -(-need // (2 * synth.BLOCK_IQ))).reshape(-1)
        rows.append(have[:need].reshape(nb, 2 * info.block_iq))
    iq = np.ascontiguousarray(np.stack(rows, axis=1))
    pipe = pkg.Pipeline(nch, mode=mode)
    fin, model = pkg.AudioFinish(nch, mode=mode), am.AudioFinish(nch, mode=mode)
    for b in range(nb):
        pipe.frontend(torch.from_numpy(iq[b]).cuda())
        lr = pipe.stereo()
        got = fin.finish(lr).cpu().numpy()
        _assert_rows(got, model.finish(lr.cpu().numpy()), f"mode {mode} block {b}")
        _assert_state(fin.state(), model.state(), f"mode {mode} block {b}")
        assert got.any()
    fin.close()
    pipe.close()


def test_from_the_pipeline(pkg, synth, torch_cuda):
    """synth.KINDS, one channel each, 10 blocks made on the GPU: frontend -> stereo -> meter.audio ->
    blend_from_meter -> finish equals the model fed the GPU's own lr and meter rows; on blocks 6-9 the
    blend target is exactly 1 with a pilot and exactly 0 without."""
    torch = torch_cuda
    kinds = list(synth.KINDS)
    nch = len(kinds)
    gen = synth.TorchMultiplexBatch(torch, nch, 0, torch.device("cuda", 0), kinds=kinds, seed=11)
    pipe, meter = pkg.Pipeline(nch), pkg.Meter(nch)
    fin, model = pkg.AudioFinish(nch), am.AudioFinish(nch)
    for b in range(NB_KINDS):
        pipe.frontend(gen.next_block())
        lr = pipe.stereo()
        meter.audio(pipe, lr)
        fin.blend_from_meter(meter)
        got = fin.finish(lr).cpu().numpy()
        rows = meter.rows()
        model.blend_from_meter(rows)
        _assert_rows(got, model.finish(lr.cpu().numpy()), f"block {b}")
        st = fin.state()
        _assert_state(st, model.state(), f"block {b}")
        if b >= 6:
            for k in ("normal", "pilot_offset", "carrier_offset"):
                assert st["blend_target"][kinds.index(k)] == 1.0, (k, b)
            for k in ("no_pilot", "noise", "silence"):
                assert st["blend_target"][kinds.index(k)] == 0.0, (k, b)
    assert (rows["flags"] & mm.ROW_AUDIO).all()
    fin.close()
    meter.close()
    pipe.close()


def test_determinism_across_batches(pkg, torch_cuda, random70):
    """Channel 37 of the batch of 70, alone: the same bytes."""
    torch = torch_cuda
    rs = np.random.Generator(np.random.PCG64(21))          # _run_random's draws, again
    fin = pkg.AudioFinish(1)
    for b in range(3):
        x = rs.integers(-32768, 32768, (70, 2 * N), dtype=np.int16)
        blend = rs.uniform(0, 1, 70).astype(np.float32)
        gain = rs.uniform(0, 2.5, 70).astype(np.float32)
        if b == 1:
            blend[0], gain[0] = 0.0, 0.0
        fin.set_control(blend[37:38], gain[37:38])
        got = fin.finish(torch.from_numpy(x[37:38]).cuda()).cpu().numpy()
        assert got.tobytes() == random70[b][0][37:38].tobytes(), f"block {b}"
        assert fin.state().tobytes() == random70[b][1][37:38].tobytes(), f"block {b}"
    fin.close()


def test_refusals_that_need_a_device(pkg, torch_cuda):
    torch = torch_cuda
    fin = pkg.AudioFinish(2)
    lr = torch.zeros(2, 2 * N + 8, dtype=torch.int16, device="cuda") + 100
    out = torch.zeros(2, 2 * N + 8, dtype=torch.int16, device="cuda")

    def refused(fn, *a, **k):
        before = fin.state()
        with pytest.raises(pkg.SdrError) as e:
            fn(*a, **k)
        assert e.value.code == -1, e.value
        assert fin.state().tobytes() == before.tobytes() and not out.any().item(), "a refused call did something"

    for other in (pkg.Meter(3), pkg.Meter(2, mode=2)):
        refused(fin.blend_from_meter, other)                    # a meter of another nch or mode
        other.close()
    L, s = pkg.lib(), None
    n2 = 2 * N
    for i_stride, o_stride in ((n2 - 2, n2 + 8), (n2 + 8, n2 - 2), (n2 + 1, n2 + 8), (n2 + 8, n2 + 3)):   # short, odd
        assert L.sdr_audio_finish(fin._h, lr.data_ptr(), i_stride, out.data_ptr(), o_stride, s) == -1
    assert L.sdr_audio_finish(fin._h, lr.data_ptr() + 2, n2 + 8, out.data_ptr(), n2 + 8, s) == -1   # 2-byte aligned base
    assert L.sdr_audio_finish(fin._h, lr.data_ptr(), n2 + 8, out.data_ptr() + 2, n2 + 8, s) == -1
    assert L.sdr_audio_finish(fin._h, None, n2 + 8, out.data_ptr(), n2 + 8, s) == -1
    refused(fin.finish, lr[:, :n2 - 2], out=out[:, :n2 - 2].contiguous())
    refused(fin.set_control, blend=[0.5, 1.5])
    refused(fin.set_control, blend=[0.5, float("nan")])
    refused(fin.set_control, gain=[-0.5, 1.0])
    refused(fin.set_control, gain=[1.0, float("inf")])
    with pytest.raises(pkg.SdrError):
        pkg.AudioFinish(2, width=3)
    torch.cuda.synchronize()
    assert not out.any().item()
    # and the accepted call next to them
    fin.set_control(blend=0.5, gain=[1.0, 0.0])
    fin.finish(lr[:, :n2], out=out[:, :n2])
    st = fin.state()
    assert st["blend"].tolist() == [0.5, 0.5] and st["gain"].tolist() == [1.0, 0.0] and out[0].any().item()
    fin.reset()
    want = am.AudioFinish(2).state()
    _assert_state(fin.state(), want, "after reset")
    fin.close()
