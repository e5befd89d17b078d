"""GPU: the multi-channel receiver with the RDS group decoder (include/sdr_multi_rds.h, sdr_multi_run_rds; the
CLI's --rds-decode) from a file: PREFIX.groups equals the model's lines (tests/rds_model.py) on the bits of
an in-process Pipeline, PREFIX.radio names the stations, the PCM and the RDS text are byte-identical to a
run without the flag, and a tuned run's khz = 0 station gives the untuned run's groups."""
from __future__ import annotations

import json
import subprocess

import numpy as np
import pytest

import rds_model as rm
from conftest import GOLD, ROOT, channel_input

pytestmark = pytest.mark.gpu

EXE = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"
NCH, NB = 4, 24


def _run(tmp_path, nch, out, *extra):
    assert EXE.exists(), "build with make"
    r = subprocess.run([str(EXE), str(nch), "--cus", "16", "--in", str(tmp_path / "in.u8"), "--out",
                        str(tmp_path / out), *extra], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    assert f"{nch} channels" in r.stderr, r.stderr
    return r


@pytest.fixture(scope="module")
def blocks(synth):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return np.stack([channel_input(synth, c, NB) for c in range(NCH)], axis=1)      # [block][channel][bytes]


@pytest.fixture(scope="module")
def model_lines(pkg, blocks):
    """The model on an in-process Pipeline's bits: the lines block after block, channels in order, and the
    channels' models."""
    import torch
    pipe = pkg.Pipeline(NCH, mode=0, rds_on=True)
    d_iq = torch.from_numpy(blocks).cuda()
    models = [rm.Channel() for _ in range(NCH)]
    lines = []
    for b in range(NB):
        pipe.frontend(d_iq[b])
        pipe.rds()
        nb, bits = pipe.nbits.cpu().numpy(), pipe.bits.cpu().numpy()
        for c in range(NCH):
            lines += [rm.group_line(c, g) for g in models[c].call(int(nb[c]), bits[c])]
    pipe.close()
    return lines, models


def test_cli_rds_decode_from_a_file(blocks, model_lines, tmp_path):
    lines, models = model_lines
    blocks.tofile(tmp_path / "in.u8")
    _run(tmp_path, NCH, "rx", "--rds-decode")
    _run(tmp_path, NCH, "plain")
    got = (tmp_path / "rx.groups").read_text().splitlines()
    assert got == lines
    fixture = json.loads((GOLD / "rds_groups_mode0.json").read_text())["channels"]
    for c in ("0", "3"):
        assert [x for x in got if x.startswith(f"ch {c} ")] == fixture[c]["groups"]
    radio = (tmp_path / "rx.radio").read_text()
    for c in range(NCH):
        assert f"ch {c}: PI: {0x1000 + c:04X}\n" in radio, radio
        s = models[c].stats()
        assert f"ch {c}: blocks: good {s['good']} corrected {s['corrected']} bad {s['bad']} BLER" in radio, radio
        assert f"ch {c}: slips: {s['slips']} sync acquired {s['acquired']} lost {s['lost']}\n" in radio, radio
        assert f"ch {c}: PTY: " in radio and f"ch {c}: groups: {s['groups']} " in radio, radio
    assert "ch 0: PS: MI355X00\n" in radio and "ch 3: PS: MI355X03\n" in radio, radio
    for ext in ("pcm", "rds"):
        assert (tmp_path / f"rx.{ext}").read_bytes() == (tmp_path / f"plain.{ext}").read_bytes(), ext
    assert (tmp_path / "rx.pcm").stat().st_size == NB * NCH * 2 * 1470 * 2
    assert not (tmp_path / "plain.groups").exists() and not (tmp_path / "plain.radio").exists()


def test_cli_rds_decode_with_tune_and_options(blocks, model_lines, tmp_path):
    """One shared capture row (channel 0's): the khz = 0 station gives the untuned run's channel 0 groups,
    with the meter, the finishing stage and --rds-correct beside it."""
    lines, _ = model_lines
    blocks[:, :1].tofile(tmp_path / "in.u8")
    (tmp_path / "tune.txt").write_text("0 0\n0 300\n")
    r = _run(tmp_path, 2, "rx", "--tune", str(tmp_path / "tune.txt"), "--rds-decode", "--rds-correct", "2", "--meter",
             "--deemph", "50")
    assert "1 capture rows per block" in r.stderr, r.stderr
    _run(tmp_path, 2, "plain", "--tune", str(tmp_path / "tune.txt"), "--meter", "--deemph", "50")
    got = (tmp_path / "rx.groups").read_text().splitlines()
    assert [x for x in got if x.startswith("ch 0 ")] == [x for x in lines if x.startswith("ch 0 ")]
    assert "ch 0: PI: 1000\n" in (tmp_path / "rx.radio").read_text()
    for ext in ("pcm", "rds", "meter", "status", "audio"):
        assert (tmp_path / f"rx.{ext}").read_bytes() == (tmp_path / f"plain.{ext}").read_bytes(), ext


def test_cli_rds_decode_on_a_wide_capture_with_the_phase_discriminator(synth, tmp_path):
    """Three blocks of the splitter tests' wide capture: too few for a group, so PREFIX.groups is empty and
    no PI is reported; the run's other files are those of the run without the decoder."""
    import split_model as spm
    wide, _ = spm.wide_composite(synth, 4, 3, (-3900, -2200, -1000))
    wide.tofile(tmp_path / "in.u8")
    (tmp_path / "tune.txt").write_text("0 -300\n1 200\n2 200\n")
    common = ("--wide", "4", "--tune", str(tmp_path / "tune.txt"), "--demod", "phase")
    r = _run(tmp_path, 3, "rx", *common, "--rds-decode", "--rds-correct", "0")
    assert "from 1 wide streams x 7 rows per block" in r.stderr, r.stderr
    _run(tmp_path, 3, "plain", *common)
    assert (tmp_path / "rx.groups").read_bytes() == b""
    radio = (tmp_path / "rx.radio").read_text()
    for c in range(3):
        assert f"ch {c}: PI: ----\n" in radio and f"ch {c}: blocks: good 0 corrected 0 bad 0 BLER 0.0000\n" in radio, radio
    for ext in ("pcm", "rds"):
        assert (tmp_path / f"rx.{ext}").read_bytes() == (tmp_path / f"plain.{ext}").read_bytes(), ext
