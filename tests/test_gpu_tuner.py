"""GPU: the shared-capture tuner (include/sdr_amd.h: sdr_tuner_set / sdr_frontend_tuned, the kernel
k_frontend_tuned of sdr_frontend.hip) against the CPU model of tests/tuner_model.py -- numpy f32
mixer, the oracle's FIR, discriminator and later stages. Everything is compared bit for bit."""
from __future__ import annotations

import sys

import numpy as np
import pytest

import tuner_model as tm
from conftest import ROOT, channel_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run_fm(pkg, torch, mode, rows, src, khz, nsrc=None):
    """fm_demod [nblocks][nch][block_if] of a tuned context over rows [nblocks][nsrc][bytes]."""
    pipe = pkg.Pipeline(len(src), mode=mode, rds_on=True)
    pipe.set_tuning(src, khz, nsrc)
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    out = []
    for b in range(rows.shape[0]):
        pipe.frontend_tuned(d[b])
        out.append(pipe.fm_demod().cpu().numpy())
    pipe.close()
    return np.stack(out)


def _mode_rows(synth, mode_block_iq: int, nblocks: int) -> np.ndarray:
    """nblocks blocks of a mode's size cut from FMMultiplexSource(0)'s byte stream (any bytes serve)."""
    need = nblocks * 2 * mode_block_iq
    have = channel_input(synth, 0, -(-need // (2 * synth.BLOCK_IQ))).reshape(-1)
    return have[:need].reshape(nblocks, 1, 2 * mode_block_iq)


def test_frontend_mode0_two_rows_six_channels(pkg, oracle, synth, torch_cuda):
    """3 blocks (block_iq mod N = 1500: a wrong per-block phase base or history mix shows at block 1,
    the parity reuse at block 2), the range edges khz = N/2 and -N/2 + 1, two rows."""
    nb = 3
    rows = np.stack([tm.composite(synth)[0][:nb], channel_input(synth, 3, nb)], axis=1)
    src, khz = [0, 0, 0, 1, 1, 0], [-600, 0, 500, 0, 1200, -1199]
    got = _run_fm(pkg, torch_cuda, 0, rows, src, khz)
    want = tm.run_tuned(pkg, oracle, 0, rows, src, khz)
    for c in range(len(src)):
        for b in range(nb):
            assert np.array_equal(_u32(got[b, c]), _u32(want[c]["fm"][b])), f"ch {c} (src {src[c]}, {khz[c]} kHz) block {b}"
    # (row 1, 0 kHz) is the untuned front end on that row
    plain = pkg.Pipeline(1)
    d = torch_cuda.from_numpy(np.ascontiguousarray(rows[:, 1:2])).cuda()
    for b in range(nb):
        plain.frontend(d[b])
        assert np.array_equal(_u32(plain.fm_demod().cpu().numpy()[0]), _u32(got[b, 3])), f"untuned block {b}"
    plain.close()


@pytest.mark.parametrize("mode,nblocks,khz", [(1, 2, (0, -301, 720)), (3, 2, (0, -301, 576)), (2, 1, (777,))])
def test_frontend_other_modes(pkg, oracle, synth, torch_cuda, mode, nblocks, khz):
    """D = 4 and 3 (N = 1440, 1152) and mode 2, which shares mode 0's front end."""
    info = pkg.Pipeline(1, mode=mode).info
    assert info.rf_Fs // 1000 == pkg.tuner_table(mode).shape[0]
    rows = _mode_rows(synth, info.block_iq, nblocks)
    src = [0] * len(khz)
    got = _run_fm(pkg, torch_cuda, mode, rows, src, list(khz))
    want = tm.run_tuned(pkg, oracle, mode, rows, src, list(khz))
    for c in range(len(khz)):
        for b in range(nblocks):
            assert np.array_equal(_u32(got[b, c]), _u32(want[c]["fm"][b])), f"mode {mode} {khz[c]} kHz block {b}"


def _check_pipeline(pkg, model, got, nb, what):
    for c in range(4):
        ref = model[c if c < 3 else 1]               # channel 3 duplicates channel 1
        for b in range(nb):
            w = f"{what}: ch {c} block {b}"
            if "fm" in got:
                assert np.array_equal(_u32(got["fm"][b][c]), _u32(ref["fm"][b])), "fm " + w
                assert np.array_equal(got["mono"][b][c], ref["mono"][b]), "mono " + w
            assert np.array_equal(got["lr"][b][c], ref["stereo"][b]), "stereo " + w
            assert np.array_equal(_u32(got["clean"][b][c]), _u32(ref["rds_clean"][b])), "rds_clean " + w
            rb = ref["bits"][b]
            if b >= 6:
                assert rb is not None, "the model decodes from block 6 on"
            if rb is None:
                assert got["nbits"][b][c] == -1, "nbits " + w
            else:
                assert got["nbits"][b][c] == len(rb), "nbits " + w
                assert np.array_equal(got["bits"][b][c, :len(rb)], rb.astype(np.uint8)), "bits " + w


def test_whole_pipeline_plain_and_persistent(pkg, oracle, synth, torch_cuda):
    """The 10-block composite: three stations and a duplicate of the middle one through every stage,
    per block on one stream, then on the persistent-PLL schedule of tests/test_gpu_width.py."""
    torch = torch_cuda
    nb = tm.COMPOSITE_BLOCKS
    comp = tm.composite(synth)[0]
    model = tm.composite_model(pkg, oracle, synth)
    src, khz = [0, 0, 0, 0], list(tm.COMPOSITE_KHZ) + [0]
    d = torch.from_numpy(np.ascontiguousarray(comp[:, None, :])).cuda()
    pipe = pkg.Pipeline(4)
    pipe.set_tuning(src, khz)
    assert pipe.nsrc == 1
    got = {k: [] for k in ("fm", "mono", "lr", "clean", "nbits", "bits")}
    for b in range(nb):
        pipe.frontend_tuned(d[b])
        got["fm"].append(pipe.fm_demod().cpu().numpy())
        got["mono"].append(pipe.mono().cpu().numpy())
        got["lr"].append(pipe.stereo().cpu().numpy())
        got["clean"].append(pipe.rds().cpu().numpy())
        got["nbits"].append(pipe.nbits.cpu().numpy().copy())
        got["bits"].append(pipe.bits.cpu().numpy().copy())
    _check_pipeline(pkg, model, got, nb, "plain")
    pipe.close()

    # persistent PLLs: plls_fits chooses the CU count, frontend_tuned for every block
    sys.path.insert(0, str(ROOT))
    import bench
    dev = torch.device("cuda", 0)
    pipe = pkg.Pipeline(4)
    pipe.set_tuning(src, khz)
    cus = bench.pll_cus(4, lambda n: pipe.plls_fits(n)["fits"])
    created: list[int] = []
    s_fe, s_pll, s_post, _ = bench.cu_masked_streams(torch, pkg, dev, str(cus), created)
    info = pipe.info
    cap = {"lr": torch.empty(nb, 4, 2 * info.n_audio, dtype=torch.int16, device=dev),
           "clean": torch.empty(nb, 4, info.n_rds, dtype=torch.float32, device=dev),
           "nbits": torch.empty(nb, 4, dtype=torch.int32, device=dev),
           "bits": torch.empty(nb, 4, pkg.SDR_MAX_BITS, dtype=torch.uint8, device=dev)}
    post_done = [torch.cuda.Event() for _ in range(nb)]
    pipe.plls_launch(nb, stream=s_pll)
    for b in range(nb):
        if b >= 2:
            s_fe.wait_event(post_done[b - 2])
        pipe.frontend_tuned(d[b], stream=s_fe)
        pipe.pre(stream=s_fe)
        pipe.plls_signal(stream=s_fe)
        pipe.plls_wait(stream=s_post)
        pipe.stereo_post(cap["lr"][b], stream=s_post)
        pipe.rds_post(cap["clean"][b], bits=True, stream=s_post)
        with torch.cuda.stream(s_post):
            cap["nbits"][b].copy_(pipe.nbits)
            cap["bits"][b].copy_(pipe.bits)
        post_done[b].record(s_post)
    torch.cuda.synchronize(dev)
    assert len(pipe.plls_report(stream=s_pll)) == nb
    host = {k: v.cpu().numpy() for k, v in cap.items()}
    pipe.close()
    bench.destroy_masked_streams(torch, pkg, dev, created)
    _check_pipeline(pkg, model, host, nb, "persistent")
    assert np.array_equal(host["lr"], np.stack(got["lr"])), "PCM differs between the schedules"
    assert np.array_equal(host["nbits"], np.stack(got["nbits"])), "bits differ between the schedules"
    assert np.array_equal(_u32(host["clean"]), _u32(np.stack(got["clean"])))


def test_refusals_reset_and_clear(pkg, oracle, synth, torch_cuda):
    torch = torch_cuda
    rows = channel_input(synth, 3, 2)[:, None, :]
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    d2 = torch.cat([d, d], dim=1)
    pipe = pkg.Pipeline(2)

    def refused(fn, *a, **k):
        with pytest.raises(pkg.SdrError) as e:
            fn(*a, **k)
        assert e.value.code == -1, e.value

    refused(pipe.frontend_tuned, d[0])                          # not tuned
    refused(pipe.set_tuning, [0, 2], [0, 0], 2)                 # src out of range
    refused(pipe.set_tuning, [0, -1], [0, 0], 1)
    refused(pipe.set_tuning, [0, 0], [0, -1200])                # khz = -N/2
    refused(pipe.set_tuning, [0, 0], [1201, 0])
    refused(pipe.set_tuning, [0, 0], [0, 0], 3)                 # nsrc > nch
    assert pipe.nsrc == 0
    pipe.set_tuning([0, 0], [0, 333])
    assert pipe.nsrc == 1
    refused(pipe.frontend, d2[0])                               # would misread the rows
    refused(pipe.frontend_pre_parts, d2[0], 4)
    pipe.frontend_tuned(d[0])
    first = pipe.fm_demod().cpu().numpy()
    refused(pipe.set_tuning, [0, 0], [0, 0])                    # a block has run
    refused(pipe.clear_tuning)
    pipe.frontend_tuned(d[1])
    # the tuning is configuration: it survives the reset, and block 0 comes out again
    pipe.reset()
    assert pipe.nsrc == 1
    pipe.frontend_tuned(d[0])
    assert np.array_equal(_u32(pipe.fm_demod().cpu().numpy()), _u32(first))
    want = tm.run_tuned(pkg, oracle, 0, rows[:1], [0, 0], [0, 333])
    for c in range(2):
        assert np.array_equal(_u32(first[c]), _u32(want[c]["fm"][0])), f"ch {c}"
    # cleared: the untuned front end again, equal to the oracle
    pipe.reset()
    pipe.clear_tuning()
    assert pipe.nsrc == 0
    refused(pipe.frontend_tuned, d[0])
    ch = oracle.Channel(0, True)
    for b in range(2):
        pipe.frontend(d2[b])
        ref = ch.frontend(rows[b, 0])
        fm = pipe.fm_demod().cpu().numpy()
        assert np.array_equal(_u32(fm[0]), _u32(ref)) and np.array_equal(_u32(fm[1]), _u32(ref)), f"block {b}"
    pipe.close()


def test_wide_1024_channels_on_128_rows(pkg, oracle, synth, torch_cuda):
    """The smallest run in which the grid order, the shared-row reads and the tile edges at full grid
    size can go wrong: 8 stations per row (negatives included), hostile rows, 2 blocks."""
    torch = torch_cuda
    nch, nsrc, nb = 1024, 128, 2
    dev = torch.device("cuda", 0)
    kinds = ["normal"] * nsrc
    hostile = [k for k in synth.KINDS if k != "normal"]
    for i, s in enumerate(np.linspace(1, nsrc - 2, len(hostile)).astype(int)):
        kinds[s] = hostile[i]
    gen = synth.TorchMultiplexBatch(torch, nsrc, 0, dev, kinds=kinds, seed=11)
    d = torch.stack([gen.next_block() for _ in range(nb)])
    offsets = [0, -1199, 1200, -600, 500, -37, 901, 250]
    # channels interleaved over the rows, so the grid order (sorted by row) is not the channel order
    src = [(7 * c) % nsrc for c in range(nch)]
    khz = [offsets[(c // nsrc + c) % 8] for c in range(nch)]
    pipe = pkg.Pipeline(nch)
    pipe.set_tuning(src, khz, nsrc)
    got = []
    for b in range(nb):
        pipe.frontend_tuned(d[b])
        got.append(pipe.fm_demod().cpu().numpy())
    pipe.close()
    # every khz = 0 channel against the untuned front end on its row
    plain = pkg.Pipeline(nsrc)
    zero = [c for c in range(nch) if khz[c] == 0]
    assert len(zero) >= 128
    for b in range(nb):
        plain.frontend(d[b])
        fm = plain.fm_demod().cpu().numpy()
        for c in zero:
            assert np.array_equal(_u32(got[b][c]), _u32(fm[src[c]])), f"khz 0 ch {c} block {b}"
    plain.close()
    # 32 channels spread over the rows, the first and the last included, against the model
    rows = d.cpu().numpy()
    picks = sorted(set(np.linspace(0, nch - 1, 32).astype(int).tolist()))
    assert picks[0] == 0 and picks[-1] == nch - 1 and len(picks) == 32
    for c in picks:
        want = tm.run_tuned(pkg, oracle, 0, rows[:, src[c]:src[c] + 1], [0], [khz[c]])[0]["fm"]
        for b in range(nb):
            assert np.array_equal(_u32(got[b][c]), _u32(want[b])), f"ch {c} (row {src[c]}, {khz[c]} kHz) block {b}"
