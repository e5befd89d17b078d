"""GPU: the multi-channel receiver with the audio finishing stage (include/sdr_multi_audio.h; the
CLI's --deemph and --blend), from a file. PREFIX.audio equals the CPU model (tests/audio_model.py) run
on that run's own PREFIX.pcm and PREFIX.meter, and every other file is byte-identical to a run
without the options."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import audio_model as am
import meter_model as mm
from conftest import ROOT

pytestmark = pytest.mark.gpu

EXE = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"
KINDS = ["normal", "silence", "carrier_offset", "no_pilot", "noise", "pilot_offset"]
NB, NCH, N = 12, len(KINDS), am.N_AUDIO


def _run(tmp, out, *extra, ok=True):
    assert EXE.exists(), "build with make"
    r = subprocess.run([str(EXE), str(NCH), "--cus", "16", "--in", str(tmp / "in.u8"), "--out", str(tmp / out), *extra],
                       capture_output=True, text=True, timeout=180)
    if ok:
        assert r.returncode == 0, r.stderr
        assert f"{NCH} channels" in r.stderr and "PLLs persistent" in r.stderr, r.stderr
    return r


@pytest.fixture(scope="module")
def runs(pkg, synth, tmp_path_factory):
    """The input file and the five runs, once."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = tmp_path_factory.mktemp("multi_audio")
    gen = synth.TorchMultiplexBatch(torch, NCH, 0, torch.device("cuda", 0), kinds=KINDS, seed=11)
    np.stack([gen.next_block().cpu().numpy() for _ in range(NB)]).tofile(tmp / "in.u8")
    _run(tmp, "plain")
    _run(tmp, "metered", "--meter")
    _run(tmp, "rx", "--meter", "--deemph", "75", "--blend")
    _run(tmp, "de50", "--deemph", "50")
    return tmp


def _pcm(path):
    raw = np.fromfile(path, np.int16)
    assert raw.size == NB * NCH * 2 * N, path
    return raw.reshape(NB, NCH, 2 * N)


def test_meter_deemph_blend(runs):
    pcm, audio = _pcm(runs / "rx.pcm"), _pcm(runs / "rx.audio")
    rows = np.frombuffer((runs / "rx.meter").read_bytes(), mm.ROW_DTYPE).reshape(NB, NCH)
    model = am.AudioFinish(NCH, tau_us=75.0)
    for b in range(NB):
        model.blend_from_meter(rows[b])
        want = model.finish(pcm[b])
        assert np.array_equal(audio[b], want), f"block {b}: {int((audio[b] != want).sum())} samples differ"
        if b >= 6:                     # no_pilot has no 19 kHz component at all: its reading is noise / noise
            assert model.g1[KINDS.index("no_pilot")] == 0.0, (b, model.g1)
    for ext in ("pcm", "rds", "meter", "status"):
        assert (runs / f"rx.{ext}").read_bytes() == (runs / f"metered.{ext}").read_bytes(), ext
    # blended to mono where there is no pilot: L = R there once the ramp has arrived and the filter settled
    tail, c = audio[8:], KINDS.index("no_pilot")
    assert np.array_equal(tail[:, c, 0::2], tail[:, c, 1::2]) and tail[:, c].any()
    assert not np.array_equal(tail[:, 0, 0::2], tail[:, 0, 1::2])


def test_deemph_alone(runs):
    pcm, audio = _pcm(runs / "de50.pcm"), _pcm(runs / "de50.audio")
    model = am.AudioFinish(NCH, tau_us=50.0)
    for b in range(NB):
        want = model.finish(pcm[b])
        assert np.array_equal(audio[b], want), f"block {b}: {int((audio[b] != want).sum())} samples differ"
    assert model.g1.tolist() == [1.0] * NCH
    for ext in ("pcm", "rds"):
        assert (runs / f"de50.{ext}").read_bytes() == (runs / f"plain.{ext}").read_bytes(), ext
    assert not (runs / "de50.meter").exists() and not (runs / "de50.status").exists()


def test_plain_and_metered_runs_write_no_audio(runs):
    assert (runs / "plain.pcm").exists() and (runs / "metered.meter").exists()
    assert not (runs / "plain.audio").exists() and not (runs / "metered.audio").exists()


def test_blend_needs_meter(runs):
    r = _run(runs, "bad", "--blend", ok=False)
    assert r.returncode != 0 and "usage: sdr_multi" in r.stderr, r.stderr
    r = _run(runs, "bad", "--deemph", "60", ok=False)
    assert r.returncode != 0 and "usage: sdr_multi" in r.stderr, r.stderr
    assert not list(runs.glob("bad.*"))
