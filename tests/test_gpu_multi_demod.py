"""GPU: the multi-channel receiver's --demod option (real-time-sdr_amd/bin/sdr_multi, the engine of
include/sdr_multi.h with SDR_FLAG_PHASE_DEMOD in sdr_multi_opts.flags). --demod phase --meter from a
file gives the Python phase pipeline's PCM and RDS text and a PREFIX.status with the deviation in kHz;
without --demod every file is the one the default path always wrote."""
from __future__ import annotations

import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, channel_input

pytestmark = pytest.mark.gpu

EXE = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"
NCH, NB = 3, 24           # the frame layer speaks after 15 decoding blocks (rds.cpp:181-189): block 21


@pytest.fixture(scope="module")
def blob(synth, tmp_path_factory):
    """[block][channel][bytes] of FMMultiplexSource(0..2), and the file that holds it."""
    iq = np.ascontiguousarray(np.stack([channel_input(synth, c, NB) for c in range(NCH)], axis=1))
    path = tmp_path_factory.mktemp("demod") / "in.u8"
    iq.tofile(path)
    return iq, path


def _run(path, out, *extra):
    assert EXE.exists(), "build with make"
    r = subprocess.run([str(EXE), str(NCH), "--cus", "16", "--in", str(path), "--out", str(out), *extra],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    assert f"{NCH} channels x {NB} blocks" in r.stderr and "PLLs persistent" in r.stderr, r.stderr
    return r


def _rds_text(tmp_path, bits) -> str:
    """The frame layer (host C++ rds_frame.cpp behind tests/cpp/rds_text_driver.cpp) on one channel's bits
    per block (None: the block decodes nothing)."""
    exe = tmp_path / "rds_text"
    if not exe.exists():
        gxx = shutil.which("g++")
        assert gxx is not None, "g++ (the host libraries are built with it)"
        subprocess.run([gxx, "-O1", "-std=c++17", "-I", str(ROOT / "include" / "dropin"),
                        str(ROOT / "tests" / "cpp" / "rds_text_driver.cpp"),
                        str(ROOT / "real-time-sdr_amd" / "host" / "rds_frame.cpp"), "-o", str(exe)], check=True)
    feed = "\n".join("-" if b is None else "".join(str(int(v)) for v in b) for b in bits) + "\n"
    return subprocess.run([str(exe)], input=feed, capture_output=True, text=True, check=True, timeout=60).stderr


def test_cli_demod_phase_with_meter(pkg, blob, tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    iq, path = blob
    _run(path, tmp_path / "rx", "--demod", "phase", "--meter")
    # the Python phase pipeline on the same bytes
    pipe = pkg.Pipeline(NCH, flags=pkg.PHASE_DEMOD)
    meter = pkg.Meter(NCH)
    d = torch.from_numpy(iq).cuda()
    pcm, bits, peaks, off = [], [[] for _ in range(NCH)], [], np.zeros(NCH)
    for b in range(NB):
        pipe.frontend(d[b])
        lr = pipe.stereo()
        pipe.rds()
        meter.audio(pipe, lr)
        dev = pkg.meter_deviation(0, meter.rows())
        peaks.append(dev["peak_khz"].copy())
        off += dev["offset_khz"]
        pcm.append(lr.cpu().numpy())
        nb_, bb = pipe.nbits.cpu().numpy(), pipe.bits.cpu().numpy()
        for c in range(NCH):
            bits[c].append(None if nb_[c] < 0 else bb[c, :nb_[c]].copy())
    meter.close()
    pipe.close()
    got = np.fromfile(tmp_path / "rx.pcm", np.int16).reshape(NB, NCH, -1)
    assert np.array_equal(got, np.stack(pcm)), "PCM differs from the Python phase pipeline's"
    text = {}
    for line in (tmp_path / "rx.rds").read_text().splitlines():
        ch, _, rest = line.partition(": ")
        text.setdefault(int(ch.split()[1]), []).append(rest)
    for c in range(NCH):
        assert "".join(ln + "\n" for ln in text.get(c, [])) == _rds_text(tmp_path, bits[c]), f"RDS text ch {c}"
        assert f"PI: {0x1000 + c:x}" in text.get(c, []), f"channel {c}: {text.get(c)}"
    lines = (tmp_path / "rx.status").read_text().splitlines()
    assert len(lines) == NCH
    peaks = np.stack(peaks)                             # [block][channel]
    peak = peaks.max(axis=0)
    # The synthetic multiplex peaks at 64.5 kHz of deviation (0.86 x 75 kHz) when all its parts align, plus
    # noise; the sine discriminator cannot read above if_Fs / 2 pi = 38.2 kHz. Block 0 is left out: the FIR
    # starts from zero history, its first outputs are a few LSBs of noise, and a step there can be any angle
    # up to pi (120 kHz) -- which is the run's maximum PREFIX.status then reports.
    assert np.all((peaks[1:] >= 45.0) & (peaks[1:] <= 75.0)), peaks
    for c, line in enumerate(lines):
        w = line.split()
        assert w[:2] == ["ch", f"{c}:"] and w[12] == "flags" and w[14] == "peak_khz" and w[16] == "offset_khz", line
        assert len(w) == 18 and "STEREO" in w[13] and "RDS" in w[13], line
        assert abs(float(w[15]) - peak[c]) <= 0.005 + 1e-9, (line, peak[c])
        assert abs(float(w[17]) - off[c] / NB) <= 0.0005 + 1e-9, (line, off[c] / NB)


def test_cli_default_is_unchanged(blob, oracle, tmp_path):
    """No --demod, and --demod ref: the same bytes in every file, the status lines without kHz fields, and
    the PCM still the oracle's (fmDemodNoArctan)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    iq, path = blob
    _run(path, tmp_path / "plain", "--meter")
    _run(path, tmp_path / "ref", "--meter", "--demod", "ref")
    for ext in ("pcm", "rds", "meter", "status"):
        a, b = (tmp_path / f"plain.{ext}").read_bytes(), (tmp_path / f"ref.{ext}").read_bytes()
        assert a == b and len(a) > 0, ext
    for line in (tmp_path / "plain.status").read_text().splitlines():
        assert "khz" not in line and len(line.split()) == 14, line
    pcm = np.fromfile(tmp_path / "plain.pcm", np.int16).reshape(NB, NCH, -1)
    ref = oracle.run_channel(iq[:, 1], 0, True)
    for b in range(NB):
        assert np.array_equal(pcm[b, 1], ref["stereo"][b]), f"stereo ch 1 block {b}"
    r = subprocess.run([str(EXE), str(NCH), "--in", str(path), "--out", str(tmp_path / "no"), "--fast", "--demod",
                        "phase"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "usage" in r.stderr and not (tmp_path / "no.pcm").exists()
