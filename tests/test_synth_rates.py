"""CPU: the synthetic multiplex generated at a mode's own sample rate (synth.TorchMultiplexBatch(fs =
rf_Fs)) is an input on which the PLLs of modes 1-3 have a pilot to lock to. The oracle's fm_demod
of block 1 (rffrontend.cpp:58-71, demod.cpp:8-19), Hann-windowed: its largest 15-23 kHz line sits
on 19 kHz and stands well clear of the band. The default-rate bytes (2.4 MS/s) read by modes 1 and
3 (1.44 and 1.152 MS/s) put the pilot near 11.4 and 9.1 kHz, outside the pilot band-pass: the same
condition fails on them, so it discriminates.

Measured with this generator (device cpu, seed 3, channels 40-43), |X| of one Hann-windowed block:
peaks 7-10 Hz off 19 kHz (the bin spacing is 27-30 Hz) at 98-810 times the band's median (dc lowest,
98-130); the default-rate bytes peak 440-2800 Hz off 19 kHz in modes 1 and 3."""
from __future__ import annotations

import numpy as np
import pytest

PILOT_KINDS = ("normal", "dc", "no_rds", "pilot_offset")
MAX_OFF_HZ = 50.0      # the largest 15-23 kHz bin lies this close to 19 kHz ...
MIN_RATIO = 50.0       # ... and is this many times the band's median


def pilot_line(fm: np.ndarray, if_fs: float) -> tuple[float, float]:
    """(distance of the largest 15-23 kHz bin from 19 kHz in Hz, its height over the band's median)."""
    n = fm.size
    spec = np.abs(np.fft.rfft(fm.astype(np.float64) * np.hanning(n)))
    f = np.arange(spec.size) * (if_fs / n)
    band = (f >= 15e3) & (f <= 23e3)
    k = int(np.argmax(spec[band]))
    return abs(float(f[band][k]) - 19e3), float(spec[band][k] / np.median(spec[band]))


def _lines(synth, oracle, mode: int, right_rate: bool) -> dict:
    import torch
    info = oracle.Channel(mode, True)
    rf_fs = int(info.state.rf_Fs)
    gen = synth.TorchMultiplexBatch(torch, len(PILOT_KINDS), first_channel=40, device="cpu", kinds=list(PILOT_KINDS),
                                    seed=3, **({"fs": rf_fs} if right_rate else {}))
    assert gen.fs == (rf_fs if right_rate else synth.FS)
    blocks = [gen.next_block(info.block_iq).numpy() for _ in range(2)]
    out = {}
    for c, kind in enumerate(PILOT_KINDS):
        ch = oracle.Channel(mode, True)
        ch.frontend(blocks[0][c])
        out[kind] = pilot_line(ch.frontend(blocks[1][c]), float(rf_fs // ch.state.rf_decim))
    return out


def _ok(line) -> bool:
    return line[0] <= MAX_OFF_HZ and line[1] >= MIN_RATIO


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_right_rate_input_has_a_pilot_at_19k(synth, oracle, mode):
    lines = _lines(synth, oracle, mode, True)
    print(f"mode {mode}: " + ", ".join(f"{k} {off:.1f} Hz x{r:.0f}" for k, (off, r) in lines.items()))
    for kind, (off, ratio) in lines.items():
        assert off <= MAX_OFF_HZ, f"mode {mode} {kind}: largest 15-23 kHz bin {off:.1f} Hz off 19 kHz"
        assert ratio >= MIN_RATIO, f"mode {mode} {kind}: pilot line only {ratio:.1f} x the band's median"


@pytest.mark.parametrize("mode", [1, 3])
def test_default_rate_input_has_no_pilot_in_modes_1_and_3(synth, oracle, mode):
    """What test_other_modes_vs_oracle feeds modes 1 and 3: no channel meets the condition."""
    lines = _lines(synth, oracle, mode, False)
    print(f"mode {mode}: " + ", ".join(f"{k} {off:.1f} Hz x{r:.0f}" for k, (off, r) in lines.items()))
    for kind, line in lines.items():
        assert not _ok(line), f"mode {mode} {kind}: {line}"


def test_fs_must_be_a_whole_rate(synth):
    with pytest.raises(ValueError):
        synth.FMMultiplexSource(0, fs=1_440_000.5)
    assert synth.FMMultiplexSource(0).fs == synth.FS
    src = synth.FMMultiplexSource(0, fs=1_152_000)
    assert src.next_block(384).shape == (768,)
