"""GPU: the RDS symbol tracker beside the pipeline and in the receiver engine (include/sdr_multi_rds.h,
sdr_multi_run_rds_clock; the CLI's --rds-clock track). RdsTracker on a Pipeline's rds_clean gives the bits of
the model (tests/rds_track_model.py) on the oracle's rds_clean; PREFIX.groups of the CLI is what the decoder's
model (tests/rds_model.py) makes of those bits, PREFIX.radio carries the clock's stats, and the PCM and the
RDS text are byte-identical to a run on the reference clock."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import rds_model as rm
import rds_track_model as tm
from conftest import ROOT, channel_input

pytestmark = pytest.mark.gpu

EXE = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"
NCH, NB = 4, 24


@pytest.fixture(scope="module")
def blocks(synth):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return np.stack([channel_input(synth, c, NB) for c in range(NCH)], axis=1)      # [block][channel][bytes]


@pytest.fixture(scope="module")
def model_bits(oracle, blocks):
    """Per channel: the tracker model's (nbits, bits) of every block on the oracle's rds_clean, and the model."""
    out = []
    for c in range(NCH):
        clean = oracle.run_channel(blocks[:, c], 0, True)["rds_clean"]
        ch = tm.Channel()
        out.append(([ch.call(row) for row in clean], ch))
    return out


def test_tracker_on_a_pipeline_equals_the_model_on_the_oracle(pkg, blocks, model_bits):
    import torch
    pipe = pkg.Pipeline(NCH, mode=0, rds_on=True)
    trk = pkg.RdsTracker(NCH)
    d_iq = torch.from_numpy(blocks).cuda()
    total = 0
    for b in range(NB):
        pipe.frontend(d_iq[b])
        clean = pipe.rds()
        nbits, bits = trk.feed_pipeline(pipe, clean)
        nb, bt = nbits.cpu().numpy(), bits.cpu().numpy()
        for c in range(NCH):
            want_n, want = model_bits[c][0][b]
            assert int(nb[c]) == want_n, (b, c)
            assert bt[c, :want_n].tolist() == want, (b, c)
            total += want_n
    stats = trk.stats()
    for c in range(NCH):
        assert {k: int(stats[c][k]) for k in tm.STATS} == model_bits[c][1].stats(), c
    assert total > NCH * 800 and all(int(s["locked"]) == 1 and int(s["resets"]) == 0 for s in stats)
    trk.close()
    pipe.close()


def _run(tmp_path, out, *extra):
    assert EXE.exists(), "build with make"
    r = subprocess.run([str(EXE), str(NCH), "--cus", "16", "--in", str(tmp_path / "in.u8"), "--out", str(tmp_path / out),
                        *extra], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_rds_clock_track_from_a_file(blocks, model_bits, tmp_path):
    blocks.tofile(tmp_path / "in.u8")
    _run(tmp_path, "trk", "--rds-decode", "--rds-clock", "track")
    _run(tmp_path, "ref", "--rds-decode", "--rds-clock", "ref")
    _run(tmp_path, "plain")
    decoders = [rm.Channel() for _ in range(NCH)]
    lines = []
    for b in range(NB):
        for c in range(NCH):
            nb, bits = model_bits[c][0][b]
            lines += [rm.group_line(c, g) for g in decoders[c].call(nb, bits)]
    got = (tmp_path / "trk.groups").read_text().splitlines()
    print(f"{len(got)} group lines on the tracker's clock, {len((tmp_path / 'ref.groups').read_text().splitlines())} on the reference's")
    assert got == lines and len(lines) >= NCH * 4
    radio = (tmp_path / "trk.radio").read_text()
    for c in range(NCH):
        s, k = decoders[c].stats(), model_bits[c][1].stats()
        assert f"ch {c}: PI: {0x1000 + c:04X}\n" in radio, radio
        assert f"ch {c}: blocks: good {s['good']} corrected {s['corrected']} bad {s['bad']} BLER" in radio, radio
        assert f"ch {c}: slips: 0 sync acquired {s['acquired']} lost {s['lost']}\n" in radio, radio
        assert (f"ch {c}: clock: locked 1 phase {k['phase']} bits {k['bits']} moves {k['moves']} half_moves {k['half_moves']} "
                f"resets 0 level {k['level']}\n") in radio, radio
    assert "clock:" not in (tmp_path / "ref.radio").read_text()
    for ext in ("pcm", "rds"):
        want = (tmp_path / f"plain.{ext}").read_bytes()
        assert (tmp_path / f"trk.{ext}").read_bytes() == want and (tmp_path / f"ref.{ext}").read_bytes() == want, ext
    assert (tmp_path / "trk.pcm").stat().st_size == NB * NCH * 2 * 1470 * 2
