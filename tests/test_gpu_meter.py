"""GPU: the reception meter (include/sdr_amd.h: sdr_meter_audio / sdr_meter_rds, the kernels of
sdr_meter.hip) against the CPU model of tests/meter_model.py. Every float field is compared as uint32
and every integer field exactly."""
from __future__ import annotations

import sys

import numpy as np
import pytest

import meter_model as mm
from conftest import ROOT, channel_input

pytestmark = pytest.mark.gpu

NB = 10


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _assert_rows(got, want, what):
    bad = mm.same_rows(got, want)
    assert not bad, f"{what}: {bad}\n got  {got}\n want {want}"


def _run_one_context(pkg, torch, mode, d, with_lr=True):
    """rows [nb][nch] (and the L/R PCM) of one context on the current stream:
    frontend -> stereo -> rds -> meter.audio(lr) -> meter.rds per block."""
    nb, nch = d.shape[0], d.shape[1]
    pipe = pkg.Pipeline(nch, mode=mode)
    meter = pkg.Meter(nch, mode=mode)
    rows, pcm = [], []
    for b in range(nb):
        pipe.frontend(d[b])
        lr = pipe.stereo()
        pipe.rds()
        meter.audio(pipe, lr if with_lr else None)
        meter.rds(pipe)
        rows.append(meter.rows())
        pcm.append(lr.cpu().numpy())
    meter.close()
    pipe.close()
    return np.stack(rows), np.stack(pcm)


@pytest.fixture(scope="module")
def kinds_run(pkg, oracle, synth, torch_cuda):
    """Mode 0, one channel per synth.KINDS entry, 10 blocks generated on the GPU and copied back for
    the model: the bytes, the GPU rows [block][kind] and the model's rows [kind][block]."""
    torch = torch_cuda
    gen = synth.TorchMultiplexBatch(torch, len(synth.KINDS), 0, torch.device("cuda", 0), kinds=synth.KINDS, seed=11)
    d = torch.stack([gen.next_block() for _ in range(NB)])
    got, pcm = _run_one_context(pkg, torch, 0, d)
    host = d.cpu().numpy()
    model = {k: mm.run_rows(oracle, 0, host[:, c]) for c, k in enumerate(synth.KINDS)}
    return {"d": d, "got": got, "model": model, "pcm": pcm}


def test_every_kind_equals_the_model(kinds_run, synth):
    """Block 1 shows the FIR history, block 2 the parity reuse, blocks >= 6 decoding beside cdr."""
    for c, kind in enumerate(synth.KINDS):
        for b in range(NB):
            _assert_rows(kinds_run["got"][b][c], kinds_run["model"][kind][b], f"{kind} block {b}")


def test_flags_of_the_kinds_on_gpu_bytes(pkg, kinds_run, synth):
    expect = {"normal": mm.STEREO | mm.RDS, "pilot_offset": mm.STEREO | mm.RDS,
              "carrier_offset": mm.STEREO | mm.RDS | mm.OFFTUNE, "no_pilot": mm.RDS, "no_rds": None, "noise": 0,
              "silence": mm.DEAD_AIR}
    for c, kind in enumerate(synth.KINDS):
        if kind not in expect:
            continue
        for b in range(6, NB):
            row = kinds_run["got"][b][c]
            f = int(pkg.meter_status(0, row)["flags"])
            assert f == mm.status(0, row)["flags"], f"{kind} block {b}"
            if expect[kind] is None:                       # no_rds: only RDS and OFFTUNE are stated
                assert not f & (mm.RDS | mm.OFFTUNE), f"{kind} block {b}: {f}"
            else:
                assert f == expect[kind], f"{kind} block {b}: {f}"
    sil = kinds_run["got"][:, list(synth.KINDS).index("silence")]
    for name in mm.ROW_DTYPE.names:
        if name not in ("flags", "eye_n"):
            assert not sil[name].any(), name


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_other_modes(pkg, oracle, synth, torch_cuda, mode):
    """Row lengths 13230, 8000, 12800 and n_rds 5105, 3087, 4940 (none a multiple of 256), symbol_Fs 20."""
    info = pkg.Pipeline(1, mode=mode).info
    nb = 2
    need = nb * 2 * info.block_iq
    have = channel_input(synth, 0, -(-need // (2 * synth.BLOCK_IQ))).reshape(-1)
    rows = np.ascontiguousarray(have[:need].reshape(nb, 1, 2 * info.block_iq))
    got, _ = _run_one_context(pkg, torch_cuda, mode, torch_cuda.from_numpy(rows).cuda())
    want = mm.run_rows(oracle, mode, rows[:, 0])
    for b in range(nb):
        _assert_rows(got[b][0], want[b], f"mode {mode} block {b}")
    assert want["eye_n"][0] > 0 and want["fm_sq"][1] > 0


def _persistent(pkg, torch, d, metered: bool):
    """The bench's three-stream persistent schedule over d [nb][4][bytes]; with `metered` both meter
    calls on the post stream after the event the front end of block b + 2 waits for, so that only the
    meter's release slots keep that front end off the rows the meter still reads."""
    sys.path.insert(0, str(ROOT))
    import bench
    dev = torch.device("cuda", 0)
    nb, nch = d.shape[0], d.shape[1]
    pipe = pkg.Pipeline(nch)
    meter = pkg.Meter(nch) if metered else None
    cus = bench.pll_cus(nch, lambda n: pipe.plls_fits(n)["fits"])
    created: list[int] = []
    s_fe, s_pll, s_post, _ = bench.cu_masked_streams(torch, pkg, dev, str(cus), created)
    info = pipe.info
    cap = {"lr": torch.empty(nb, nch, 2 * info.n_audio, dtype=torch.int16, device=dev),
           "clean": torch.empty(nb, nch, info.n_rds, dtype=torch.float32, device=dev),
           "nbits": torch.empty(nb, nch, dtype=torch.int32, device=dev),
           "bits": torch.empty(nb, nch, pkg.SDR_MAX_BITS, dtype=torch.uint8, device=dev),
           "rows": torch.zeros(nb, nch * 64, dtype=torch.uint8, device=dev)}
    post_done = [torch.cuda.Event() for _ in range(nb)]
    pipe.plls_launch(nb, stream=s_pll)
    for b in range(nb):
        if b >= 2:
            s_fe.wait_event(post_done[b - 2])
        pipe.frontend(d[b], stream=s_fe)
        pipe.pre(stream=s_fe)
        pipe.plls_signal(stream=s_fe)
        pipe.plls_wait(stream=s_post)
        pipe.stereo_post(cap["lr"][b], stream=s_post)
        pipe.rds_post(cap["clean"][b], bits=True, stream=s_post)
        with torch.cuda.stream(s_post):
            cap["nbits"][b].copy_(pipe.nbits)
            cap["bits"][b].copy_(pipe.bits)
        post_done[b].record(s_post)
        if metered:
            meter.audio(pipe, cap["lr"][b], stream=s_post)
            meter.rds(pipe, stream=s_post)
            meter.rows_into(cap["rows"][b], stream=s_post)
    torch.cuda.synchronize(dev)
    assert len(pipe.plls_report(stream=s_pll)) == nb
    host = {k: v.cpu().numpy() for k, v in cap.items()}
    host["rows"] = host["rows"].view(mm.ROW_DTYPE).reshape(nb, nch)
    if meter:
        meter.close()
    pipe.close()
    bench.destroy_masked_streams(torch, pkg, dev, created)
    return host


def test_persistent_schedule(pkg, kinds_run, synth, torch_cuda):
    """4 channels, 10 blocks: the rows equal the plain schedule's, and the PCM and bits equal an
    unmetered run of the same schedule (the new release slots change nothing they should not)."""
    kinds = list(synth.KINDS)
    pick = [kinds.index(k) for k in ("normal", "carrier_offset", "no_pilot", "pilot_offset")]
    d = kinds_run["d"][:, pick].contiguous()
    metered = _persistent(pkg, torch_cuda, d, True)
    plain = _persistent(pkg, torch_cuda, d, False)
    for b in range(NB):
        for i, c in enumerate(pick):
            _assert_rows(metered["rows"][b][i], kinds_run["got"][b][c], f"{kinds[c]} block {b}")
    assert np.array_equal(metered["lr"], plain["lr"]), "PCM differs from the unmetered run"
    assert np.array_equal(metered["lr"], kinds_run["pcm"][:, pick]), "PCM differs from the plain schedule"
    assert np.array_equal(metered["nbits"], plain["nbits"]) and np.array_equal(metered["bits"], plain["bits"])
    assert np.array_equal(metered["clean"].view(np.uint32), plain["clean"].view(np.uint32))
    assert not plain["rows"].view(np.uint8).any()


def test_two_contexts_joined_by_push(pkg, kinds_run, synth, torch_cuda):
    """The engine's shape: the audio chain on one context and stream, the RDS chain on another that
    takes the block through push_fm_demod; both calls fill one meter's rows."""
    torch = torch_cuda
    d = kinds_run["d"]
    nch = d.shape[1]
    audio, rds = pkg.Pipeline(nch), pkg.Pipeline(nch)
    meter = pkg.Meter(nch)
    s_rds = torch.cuda.Stream()
    fm = [torch.empty(nch, audio.info.block_if, dtype=torch.float32, device=d.device) for _ in range(2)]
    for b in range(NB):
        if b >= 2:
            torch.cuda.current_stream().wait_stream(s_rds)     # fm[b % 2] is the caller's to order
        audio.frontend(d[b])
        audio.fm_demod(fm[b % 2])
        s_rds.wait_stream(torch.cuda.current_stream())
        lr = audio.stereo()
        meter.audio(audio, lr)
        rds.push_fm_demod(fm[b % 2], stream=s_rds)
        rds.rds(stream=s_rds)
        meter.rds(rds, stream=s_rds)
        torch.cuda.current_stream().synchronize()
        rows = meter.rows(stream=s_rds)
        for c, kind in enumerate(synth.KINDS):
            _assert_rows(rows[c], kinds_run["got"][b][c], f"{kind} block {b}")
    meter.close()
    audio.close()
    rds.close()


def test_wide_1024_channels(pkg, oracle, synth, torch_cuda):
    """Full grid width, hostile kinds spread over the rows, 2 blocks: 32 channels from the first to the
    last against the model, and every silence row all zero."""
    torch = torch_cuda
    nch, nb = 1024, 2
    kinds = ["normal"] * nch
    hostile = [k for k in synth.KINDS if k != "normal"]
    for i in range(nch // 8):
        kinds[8 * i + 3] = hostile[i % len(hostile)]
    kinds[0], kinds[nch - 1] = "silence", "noise"
    gen = synth.TorchMultiplexBatch(torch, nch, 0, torch.device("cuda", 0), kinds=kinds, seed=11)
    d = torch.stack([gen.next_block() for _ in range(nb)])
    got, _ = _run_one_context(pkg, torch, 0, d)
    picks = sorted(set(np.linspace(0, nch - 1, 32).astype(int).tolist()) | {3, 11})
    assert picks[0] == 0 and picks[-1] == nch - 1
    for c in picks:
        want = mm.run_rows(oracle, 0, d[:, c].cpu().numpy())
        for b in range(nb):
            _assert_rows(got[b][c], want[b], f"ch {c} ({kinds[c]}) block {b}")
    sil = got[:, [c for c in range(nch) if kinds[c] == "silence"]]
    assert sil.shape[1] >= 12
    for name in mm.ROW_DTYPE.names:
        if name not in ("flags", "eye_n"):
            assert not sil[name].any(), name
    assert (sil["flags"] == 3).all() and (sil["eye_n"] == 73).all()


def test_refusals_null_lr_and_reset(pkg, oracle, synth, torch_cuda):
    torch = torch_cuda
    iq = np.ascontiguousarray(channel_input(synth, 3, 2)[:, None, :].repeat(2, axis=1))
    d = torch.from_numpy(iq).cuda()
    pipe = pkg.Pipeline(2)
    meter = pkg.Meter(2)
    info = pipe.info

    def refused(fn, *a, **k):
        before = meter.rows()
        with pytest.raises(pkg.SdrError) as e:
            fn(*a, **k)
        assert e.value.code == -1, e.value
        assert meter.rows().tobytes() == before.tobytes(), "a refused call touched the rows"

    refused(meter.audio, pipe)                                  # no block yet
    refused(meter.rds, pipe)
    pipe.frontend(d[0])
    refused(meter.audio, pipe)                                  # stereo_pre has not run
    refused(meter.rds, pipe)                                    # nor the RDS stages
    pipe.stereo_pre()
    refused(meter.rds, pipe)
    lr = torch.zeros(2, 2 * info.n_audio, dtype=torch.int16, device=d.device)
    refused(meter.audio, pipe, lr[:, :2 * info.n_audio - 2].contiguous())   # short lr_stride
    pipe.rds_pre()
    refused(meter.rds, pipe)                                    # rds_pre alone is not enough
    for other in (pkg.Pipeline(3), pkg.Pipeline(2, mode=2), pkg.Pipeline(2, rds_on=False)):
        other.frontend(torch.zeros(other.nch, 2 * other.info.block_iq, dtype=torch.uint8, device=d.device) + 128)
        other.stereo()
        if other.info.rds_on:
            other.rds()
            refused(meter.audio, other)                         # another nch or mode
            refused(meter.rds, other)
        else:
            refused(meter.rds, other)                           # no RDS chain
        other.close()
    assert not meter.rows().view(np.uint8).any()

    # lr = None: the audio fields stay 0, the audio bit is set; only that part is written
    pipe.stereo_pll()
    pipe.stereo_post(lr)
    meter.audio(pipe, None)
    row = meter.rows()
    ref = mm.ChannelMeter(oracle, 0)
    want, want_lr, _ = ref.block(iq[0, 0], with_lr=False)
    want["flags"] = mm.ROW_AUDIO
    for name in ("rds_sq", "eye_abs", "eye_sq", "eye_n"):
        want[name] = 0
    for c in range(2):
        _assert_rows(row[c], want, f"lr = None, ch {c}")
    assert row["fm_sq"][0] > 0 and not row["l_sq"].any() and not row["l_peak"].any()
    assert np.array_equal(lr.cpu().numpy()[0], want_lr)
    # the same block again with its PCM, on a fresh meter: the integers too
    meter2 = pkg.Meter(2)
    meter2.audio(pipe, lr)
    ref2 = mm.ChannelMeter(oracle, 0)
    want2 = ref2.block(iq[0, 0])[0]
    got2 = meter2.rows()
    assert got2["l_sq"][0] == want2["l_sq"] > 0 and got2["r_peak"][1] == want2["r_peak"] > 0
    meter2.close()
    # reset clears the rows
    meter.reset()
    assert not meter.rows().view(np.uint8).any()
    meter.close()
    pipe.close()
