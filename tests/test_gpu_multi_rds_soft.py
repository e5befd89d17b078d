"""GPU: RDS soft decisions in the receiver engine (include/sdr_multi_rds.h, sdr_multi_run_rds_soft; the CLI's
--rds-soft L). PREFIX.groups and PREFIX.radio of a run with --rds-soft 6 are what the models of
tests/rds_soft_model.py make of the oracle's rds_clean, every other file is that of the run without the option,
and the run without it is what the hard decoder's model (tests/rds_model.py) makes of the tracker's bits."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import rds_model as rm
import rds_soft_model as sm
from conftest import ROOT

pytestmark = pytest.mark.gpu

EXE = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"
NB = 30
STATIONS = ((0, 0.85, 0.01), (0, 0.02, 0.01), (5, 0.03, 0.01), (7, 0.03, 0.02))     # (synth channel, iq_amplitude, noise)
NCH = len(STATIONS)


@pytest.fixture(scope="module")
def blocks(synth):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    srcs = [synth.FMMultiplexSource(c, iq_amplitude=a, noise=n) for c, a, n in STATIONS]
    return np.stack([np.stack([s.next_block() for s in srcs]) for _ in range(NB)])      # [block][channel][bytes]


@pytest.fixture(scope="module")
def model_calls(oracle, blocks):
    """Per channel: the soft tracker model's (nbits, bits, soft) of every block on the oracle's rds_clean."""
    out = []
    for c in range(NCH):
        clean = oracle.run_channel(blocks[:, c], 0, True)["rds_clean"]
        ch = sm.TrackChannel()
        out.append([ch.call(row) for row in clean])
    return out


def _run(tmp_path, out, *extra):
    assert EXE.exists(), "build with make"
    r = subprocess.run([str(EXE), str(NCH), "--cus", "16", "--in", str(tmp_path / "in.u8"), "--out", str(tmp_path / out),
                        *extra], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    return r


def _model_lines(model_calls, decoders, line):
    lines = []
    for b in range(NB):
        for c in range(NCH):
            nb, bits, soft = model_calls[c][b]
            groups = decoders[c].call(nb, bits, soft) if isinstance(decoders[c], sm.Channel) else decoders[c].call(nb, bits)
            lines += [line(c, g) for g in groups]
    return lines


def test_cli_rds_soft_from_a_file(blocks, model_calls, tmp_path):
    blocks.tofile(tmp_path / "in.u8")
    _run(tmp_path, "soft", "--rds-decode", "--rds-clock", "track", "--rds-soft", "6", "--meter")
    _run(tmp_path, "hard", "--rds-decode", "--rds-clock", "track", "--meter")
    soft = [sm.Channel(soft_bits=6) for _ in range(NCH)]
    hard = [rm.Channel() for _ in range(NCH)]
    soft_lines = _model_lines(model_calls, soft, sm.group_line)
    hard_lines = _model_lines(model_calls, hard, rm.group_line)
    # with the option: the soft models' lines
    got = (tmp_path / "soft.groups").read_text().splitlines()
    assert got == soft_lines and sum("~" in ln for ln in got) >= 5
    radio = (tmp_path / "soft.radio").read_text()
    for c in range(NCH):
        s = soft[c].stats()
        assert f"ch {c}: blocks: good {s['good']} corrected {s['corrected']} bad {s['bad']} BLER" in radio, radio
        assert f"ch {c}: soft: blocks {soft[c].soft_blocks} flips {soft[c].soft_flips}\n" in radio, radio
    assert radio.count(" soft: ") == NCH and radio.count(" clock: ") == NCH
    assert sum(ch.soft_blocks for ch in soft) >= 5 and soft[0].soft_blocks == 0
    print("soft blocks per channel:", [ch.soft_blocks for ch in soft], "bad hard/soft:", [ch.bad for ch in hard], [ch.bad for ch in soft])
    # without it: the hard model's lines, no trace of the soft step
    assert (tmp_path / "hard.groups").read_text().splitlines() == hard_lines
    hard_radio = (tmp_path / "hard.radio").read_text()
    assert "soft:" not in hard_radio and "~" not in (tmp_path / "hard.groups").read_text()
    for c in range(NCH):
        s = hard[c].stats()
        assert f"ch {c}: blocks: good {s['good']} corrected {s['corrected']} bad {s['bad']} BLER" in hard_radio, hard_radio
    # the clock lines are the same, and so is every other file
    clock = [ln for ln in radio.splitlines() if " clock: " in ln]
    assert clock == [ln for ln in hard_radio.splitlines() if " clock: " in ln]
    others = sorted(p.name.split(".", 1)[1] for p in tmp_path.glob("hard.*") if p.suffix not in (".groups", ".radio"))
    assert {"pcm", "rds", "meter", "status"} <= set(others), others
    for ext in others:
        assert (tmp_path / f"soft.{ext}").read_bytes() == (tmp_path / f"hard.{ext}").read_bytes(), ext
    assert sorted(p.name.split(".", 1)[1] for p in tmp_path.glob("soft.*")) == sorted(others + ["groups", "radio"])
