"""GPU: the phase discriminator (SDR_FLAG_PHASE_DEMOD, include/sdr_amd.h; the PH instantiations of
k_frontend2, k_frontend_tuned and k_demod) against its definition tests/demod_model.py -- the oracle's
FIR outputs of the same bytes (the tuner model's mixer in front of them, khz = 0 being the identity),
then demod_model.demod. Everything is compared bit for bit unless said otherwise.

Not covered: the generic k_frontend<true>. A context always has 101 taps and a decimation of 10, 4 or
3, so none dispatches the generic kernel, with or without the flag; it has no GPU test of its own."""
from __future__ import annotations

import sys

import numpy as np
import pytest

import demod_model as dm
import tuner_model as tm
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


class PhaseChannel(tm.TunedChannel):
    """The tuner model's channel with the phase discriminator behind the oracle's FIR."""

    def frontend(self, row, iq):
        n0 = self.block * self.block_iq
        hi, hq = self._mix(row.tail, n0 - (tm.NTAPS - 1))
        yi, yq = self._mix(iq, n0)
        I = self.oracle.fir_decim(yi, self.h, np.ascontiguousarray(hi), self.D)
        Q = self.oracle.fir_decim(yq, self.h, np.ascontiguousarray(hq), self.D)
        fm, self.prev = dm.demod(I, Q, self.prev)
        self.block += 1
        return fm


def phase_model(pkg, oracle, mode, rows, src, khz):
    """fm [nch][nblocks][block_if] of the model over rows u8 [nblocks][nsrc][2*block_iq]."""
    chans = [PhaseChannel(pkg, oracle, mode, k) for k in khz]
    srows = [tm.TunedRow() for _ in range(rows.shape[1])]
    out = [[] for _ in chans]
    for b in range(rows.shape[0]):
        for c, ch in enumerate(chans):
            out[c].append(ch.frontend(srows[src[c]], rows[b, src[c]]))
        for r, sr in enumerate(srows):
            sr.tail = rows[b, r, -2 * (tm.NTAPS - 1):].copy()
    return out


def _gen(torch, synth, pkg, mode, kinds, nblocks, seed):
    """u8 [nblocks][nch][2*block_iq] generated on the device at the mode's own rf_Fs."""
    info = pkg.Pipeline(1, mode=mode).info
    gen = synth.TorchMultiplexBatch(torch, len(kinds), 0, torch.device("cuda", 0), kinds=list(kinds), seed=seed,
                                    fs=info.rf_Fs)
    return torch.stack([gen.next_block(info.block_iq) for _ in range(nblocks)])


def _run_phase(pkg, d, mode, flags):
    pipe = pkg.Pipeline(d.shape[1], mode=mode, rds_on=True, flags=flags)
    out = []
    for b in range(d.shape[0]):
        pipe.frontend(d[b])
        out.append(pipe.fm_demod().cpu().numpy())
    pipe.close()
    return np.stack(out)


@pytest.fixture(scope="module")
def mode0_kinds(pkg, oracle, synth, torch_cuda):
    """Mode 0, one channel per synth kind, 3 blocks: (device bytes, host bytes, the phase context's fm)."""
    d = _gen(torch_cuda, synth, pkg, 0, synth.KINDS, 3, seed=41)
    return d, d.cpu().numpy(), _run_phase(pkg, d, 0, pkg.PHASE_DEMOD)


def test_frontend_mode0_every_kind_equals_model(pkg, oracle, synth, mode0_kinds):
    """k_frontend2<8, 10, true>: silence is mx == 0 throughout, block 0 starts from the zero carry, blocks 1
    and 2 from the carried sample of either parity."""
    assert len(synth.KINDS) == 11
    _, rows, got = mode0_kinds
    nch = rows.shape[1]
    want = phase_model(pkg, oracle, 0, rows, list(range(nch)), [0] * nch)
    for c, kind in enumerate(synth.KINDS):
        for b in range(rows.shape[0]):
            assert np.array_equal(_u32(got[b, c]), _u32(want[c][b])), f"{kind} block {b}"
    sil = synth.KINDS.index("silence")
    assert not got[:, sil].any() and not np.signbit(got[:, sil]).any()
    assert np.all(np.abs(got) <= dm.PI)
    # the folded station: the phase context reads well beyond the sine's range on carrier_offset
    assert np.max(np.abs(got[1:, synth.KINDS.index("carrier_offset")])) > 1.6


def test_default_context_still_equals_the_reference(pkg, oracle, mode0_kinds):
    """Without the flag the same bytes still give fmDemodNoArctan, and FAST | PHASE is refused."""
    d, rows, got = mode0_kinds
    plain = _run_phase(pkg, d, 0, 0)
    for c in range(rows.shape[1]):
        ch = oracle.Channel(0, True)
        for b in range(rows.shape[0]):
            assert np.array_equal(_u32(plain[b, c]), _u32(ch.frontend(rows[b, c]))), f"ch {c} block {b}"
    assert not np.array_equal(_u32(plain[:, 0]), _u32(got[:, 0]))
    with pytest.raises(pkg.SdrError) as e:
        pkg.Pipeline(2, flags=pkg.FLAG_FAST_FRONTEND | pkg.PHASE_DEMOD)
    assert e.value.code == -1, e.value


@pytest.mark.parametrize("mode", [1, 3])
def test_frontend_other_decimations_equal_model(pkg, oracle, synth, torch_cuda, mode):
    """D = 4 and 3 (k_frontend2<8, 4, true>, <8, 3, true>) on bytes at the mode's own rate."""
    d = _gen(torch_cuda, synth, pkg, mode, ("normal", "carrier_offset"), 2, seed=43 + mode)
    rows = d.cpu().numpy()
    got = _run_phase(pkg, d, mode, pkg.PHASE_DEMOD)
    want = phase_model(pkg, oracle, mode, rows, [0, 1], [0, 0])
    for c in range(2):
        for b in range(2):
            assert np.array_equal(_u32(got[b, c]), _u32(want[c][b])), f"mode {mode} ch {c} block {b}"


def test_frontend_pre_parts_equals_whole_block(pkg, mode0_kinds, torch_cuda):
    """The pipeline fill's tile-range launches (sdr_frontend_pre_parts, 4 parts) of a phase context give
    the whole-block launch's fm rows, and the block behind it continues from the same carry."""
    torch = torch_cuda
    sys.path.insert(0, str(ROOT))
    import bench
    d, _, whole = mode0_kinds
    nch, dev = d.shape[1], torch.device("cuda", 0)
    pipe = pkg.Pipeline(nch, flags=pkg.PHASE_DEMOD)
    cus = bench.pll_cus(nch, lambda n: pipe.plls_fits(n)["fits"])
    created: list[int] = []
    try:
        s_fe, s_pll, s_post, _ = bench.cu_masked_streams(torch, pkg, dev, str(cus), created)
    except (RuntimeError, AttributeError):
        pipe.close()
        pytest.skip("no CU-masked streams: the persistent PLL launch needs them")
    info = pipe.info
    fm = torch.empty(2, nch, info.block_if, dtype=torch.float32, device=dev)
    lr = torch.empty(2, nch, 2 * info.n_audio, dtype=torch.int16, device=dev)
    clean = torch.empty(2, nch, info.n_rds, dtype=torch.float32, device=dev)
    pipe.plls_launch(2, stream=s_pll)
    for b in range(2):
        if b == 0:
            pipe.frontend_pre_parts(d[b], 4, stream=s_fe)
        else:
            pipe.frontend(d[b], stream=s_fe)
            pipe.pre(stream=s_fe)
            pipe.plls_signal(stream=s_fe)
        pipe.fm_demod(fm[b], stream=s_fe)
        pipe.plls_wait(stream=s_post)
        pipe.stereo_post(lr[b], stream=s_post)
        pipe.rds_post(clean[b], bits=True, stream=s_post)
    torch.cuda.synchronize(dev)
    assert len(pipe.plls_report(stream=s_pll)) == 2
    got = fm.cpu().numpy()
    pipe.close()
    bench.destroy_masked_streams(torch, pkg, dev, created)
    for b in range(2):
        assert np.array_equal(_u32(got[b]), _u32(whole[b])), f"block {b}"


def test_tuned_four_stations_on_two_rows(pkg, oracle, synth, mode0_kinds, torch_cuda):
    """k_frontend_tuned<4, 10, true>: the tuner model's mixed samples, the FIR, then the phase model;
    the khz = 0 station equals the untuned phase context on its row."""
    torch = torch_cuda
    d, rows, whole = mode0_kinds
    sel = [synth.KINDS.index("normal"), synth.KINDS.index("dc")]
    rows2 = np.ascontiguousarray(rows[:2, sel])
    src, khz = [0, 0, 1, 1], [0, 300, -600, 1]
    pipe = pkg.Pipeline(4, flags=pkg.PHASE_DEMOD)
    pipe.set_tuning(src, khz, 2)
    d2 = torch.from_numpy(rows2).cuda()
    got = []
    for b in range(2):
        pipe.frontend_tuned(d2[b])
        got.append(pipe.fm_demod().cpu().numpy())
    pipe.close()
    want = phase_model(pkg, oracle, 0, rows2, src, khz)
    for c in range(4):
        for b in range(2):
            assert np.array_equal(_u32(got[b][c]), _u32(want[c][b])), f"ch {c} ({khz[c]} kHz) block {b}"
    for b in range(2):
        assert np.array_equal(_u32(got[b][0]), _u32(whole[b, sel[0]])), f"khz 0 against the untuned context, block {b}"


def _group_bits(synth, channel: int) -> np.ndarray:
    """The four 0A groups channel `channel` repeats, as bits before the differential encoding."""
    pty, ps = (channel * 7 + 10) % 32, f"MI355X{channel % 100:02d}"
    return np.array([(blk >> (25 - i)) & 1 for seg in range(4)
                     for blk in synth.rds_group_0a(0x1000 + channel, pty, seg, ps) for i in range(26)], np.uint8)


def test_rest_of_the_pipeline_is_untouched(pkg, synth, torch_cuda):
    """3 channels x 8 blocks: a phase context end to end, and a default context fed the phase context's
    fm rows (sdr_get_fm_demod -> sdr_push_fm_demod): mono, stereo, rds_clean and the bits are identical, so
    the flag changes the discriminator and nothing behind it. The decoded bits are the channel's own
    groups (PI 0x1000 + channel; the PI text itself needs 21 blocks: tests/test_gpu_multi_demod.py)."""
    nch, nb = 3, 8
    d = _gen(torch_cuda, synth, pkg, 0, ("normal",) * nch, nb, seed=47)
    a = pkg.Pipeline(nch, flags=pkg.PHASE_DEMOD)
    p = pkg.Pipeline(nch)
    decoded = 0
    for b in range(nb):
        a.frontend(d[b])
        fm = a.fm_demod()
        p.push_fm_demod(fm)
        for name in ("mono", "stereo", "rds"):
            x, y = getattr(a, name)().cpu().numpy(), getattr(p, name)().cpu().numpy()
            assert x.tobytes() == y.tobytes(), f"{name} block {b}"
        na, npl = a.nbits.cpu().numpy(), p.nbits.cpu().numpy()
        assert np.array_equal(na, npl) and np.array_equal(a.bits.cpu().numpy(), p.bits.cpu().numpy()), f"bits block {b}"
        assert np.all((na >= 0) == (b >= 6)), f"block {b}: nbits {na}"
        if b >= 6:
            bits = a.bits.cpu().numpy()
            for c in range(nch):
                run = "".join(map(str, bits[c, 1:na[c]]))           # bit 0 depends on the block before
                assert len(run) >= 30
                own = ["".join(map(str, np.tile(_group_bits(synth, k), 2))) for k in range(nch)]
                assert run in own[c], f"channel {c} block {b}: not its own groups"
                assert all(run not in own[k] for k in range(nch) if k != c)
                decoded += 1
    assert decoded == 2 * nch
    a.close()
    p.close()


@pytest.mark.parametrize("n", [1, 63, 513])
def test_primitive_ragged_lengths(pkg, torch_cuda, n):
    """sdr_fm_demod_phase on random f32 I/Q, 3 rows with a row stride beyond n, two calls (the carry)."""
    torch = torch_cuda
    rng = np.random.default_rng(100 + n)
    nch, stride = 3, n + 5
    I, Q = (rng.standard_normal((2, nch, stride)).astype(np.float32) * np.float32(0.3) for _ in range(2))
    I[0, 1, :n // 2] = 0                                            # zero samples: mx == 0 and a zero previous one
    Q[0, 1, :n // 2] = 0
    prev = torch.zeros(nch, 2, dtype=torch.float32, device="cuda")
    mprev = np.zeros((nch, 2), np.float32)
    for k in range(2):
        dI, dQ = torch.from_numpy(I[k]).cuda()[:, :n], torch.from_numpy(Q[k]).cuda()[:, :n]
        out = torch.full((nch, stride), 9.0, dtype=torch.float32, device="cuda")[:, :n]
        pkg.fm_demod_phase(out, dI, dQ, prev)
        want, mprev = dm.demod(I[k][:, :n], Q[k][:, :n], mprev)
        assert np.array_equal(_u32(out.cpu().numpy()), _u32(want)), f"call {k}"
        assert np.array_equal(_u32(prev.cpu().numpy()), _u32(mprev)), f"prev after call {k}"
    assert np.array_equal(pkg.demod_coeffs(), dm.COEFFS)


def test_tone_75khz_on_the_device(pkg, torch_cuda):
    """The loud tone of tests/test_demod_model.py through the phase front end: HD3 <= -60 dB, fundamental
    within 1 % and the meter's peak 75 +- 1.5 kHz; the default context folds it (HD3 above -20 dB)."""
    torch = torch_cuda
    u8 = dm.tone_iq(75.0, 2 * 73500).reshape(2, 1, -1)
    d = torch.from_numpy(u8).cuda()
    fm = {}
    for flags in (pkg.PHASE_DEMOD, 0):
        pipe = pkg.Pipeline(1, flags=flags)
        meter = pkg.Meter(1)
        rows = []
        for b in range(2):
            pipe.frontend(d[b])
            rows.append(pipe.fm_demod().cpu().numpy()[0])
            lr = pipe.stereo()
            meter.audio(pipe, lr)
        row = meter.rows()                                          # block 1: past the FIR's start-up
        fm[flags] = np.concatenate(rows)
        if flags:
            dev_khz = pkg.meter_deviation(0, row)[0]
        meter.close()
        pipe.close()
    r = dm.tone_readings(fm[pkg.PHASE_DEMOD])
    print(f"device, phase: {r}; meter: {dev_khz}")
    assert r["hd3_db"] <= -60.0
    assert abs(r["fund"] / (2.0 * np.pi * 75.0 / 240.0) - 1.0) <= 0.01
    assert abs(r["peak_khz"] - 75.0) <= 1.5
    assert abs(dev_khz["peak_khz"] - 75.0) <= 1.5
    assert abs(dev_khz["offset_khz"]) <= 1.0 and 50.0 <= dev_khz["rms_khz"] <= 56.0    # 75 / sqrt(2) = 53.0
    s = dm.tone_readings(fm[0])
    print(f"device, default: {s}")
    assert s["hd3_db"] > -20.0
