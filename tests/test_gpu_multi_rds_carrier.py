"""GPU: coherent RDS in the receiver engine (include/sdr_multi_rds.h, sdr_multi_run_rds_carrier; the CLI's
--rds-carrier quad). PREFIX.groups and PREFIX.radio of such a run are what the models make of the oracle's rows:
the quadrature branch (tests/rds_quad_model.py), the derotator (tests/rds_carrier_model.py), the tracker and the
decoders; PREFIX.radio carries the carrier's stats, and every other file is byte-identical to the run on the
tracker's clock without the option. --rds-soft 6 works on top."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import rds_carrier_model as cm
import rds_model as rm
import rds_quad_model as qm
import rds_soft_model as sm
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
def model_calls(oracle, blocks):
    """Per channel: the soft tracker model's (nbits, bits, soft) of every block on the derotator model's rows of
    the oracle's two branches, the tracker's model and the derotator's."""
    out = []
    for c in range(NCH):
        rows = qm.run_channel(oracle, blocks[:, c])
        car, trk = cm.Channel(), sm.TrackChannel()
        calls = [trk.call(car.call(xi, xq)) for xi, xq in zip(rows["rds_clean"], rows["rds_clean_q"])]
        out.append((calls, trk, car))
    return out


def test_derotator_on_a_pipeline_equals_the_models_on_the_oracle(pkg, blocks, model_calls):
    """Pipeline(flags=RDS_QUAD), RdsCarrier.feed_pipeline on the context's own quadrature rows, RdsTracker on the
    rotated rows: the bits, reliabilities and both handles' stats of the models on the oracle's rows."""
    import torch
    pipe = pkg.Pipeline(NCH, mode=0, rds_on=True, flags=pkg.RDS_QUAD)
    car, trk = pkg.RdsCarrier(NCH), pkg.RdsTracker(NCH)
    d_iq = torch.from_numpy(blocks).cuda()
    total = 0
    for b in range(NB):
        pipe.frontend(d_iq[b])
        rows = car.feed_pipeline(pipe, pipe.rds())
        nbits, bits, soft = trk.feed(rows, pipe.info.n_rds, soft=True)
        nb, bt, sf = nbits.cpu().numpy(), bits.cpu().numpy(), soft.cpu().numpy().view(np.uint16)
        for c in range(NCH):
            want_n, want, want_soft = model_calls[c][0][b]
            assert int(nb[c]) == want_n, (b, c)
            assert bt[c, :want_n].tolist() == list(want) and sf[c, :want_n].tolist() == list(want_soft), (b, c)
            total += want_n
    cs, ts = car.stats(), trk.stats()
    for c in range(NCH):
        assert {k: int(cs[c][k]) for k in cm.STATS} == model_calls[c][2].stats(), c
        assert int(ts[c]["bits"]) == model_calls[c][1].stats()["bits"] and int(ts[c]["locked"]) == 1
    assert total > NCH * 800
    assert np.all(np.abs(pkg.rds_carrier_phase_deg(cs) + 45.0) < 10.0) and np.all(pkg.rds_carrier_coherence(cs) > 0.9)
    for h in (car, trk, pipe):
        h.close()


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
            nb, bits, soft = model_calls[c][0][b]
            groups = decoders[c].call(nb, bits, soft) if isinstance(decoders[c], sm.Channel) else decoders[c].call(nb, bits)
            lines += [line(c, g) for g in groups]
    return lines


def test_cli_rds_carrier_quad_from_a_file(blocks, model_calls, tmp_path):
    blocks.tofile(tmp_path / "in.u8")
    _run(tmp_path, "quad", "--rds-decode", "--rds-clock", "track", "--rds-carrier", "quad", "--meter")
    _run(tmp_path, "soft", "--rds-decode", "--rds-clock", "track", "--rds-carrier", "quad", "--rds-soft", "6", "--meter")
    _run(tmp_path, "trk", "--rds-decode", "--rds-clock", "track", "--rds-carrier", "ref", "--meter")
    hard = [rm.Channel() for _ in range(NCH)]
    soft = [sm.Channel(soft_bits=6) for _ in range(NCH)]
    hard_lines = _model_lines(model_calls, hard, rm.group_line)
    soft_lines = _model_lines(model_calls, soft, sm.group_line)
    got = (tmp_path / "quad.groups").read_text().splitlines()
    print(f"{len(got)} group lines on the derotated rows, {len((tmp_path / 'trk.groups').read_text().splitlines())} on rds_clean")
    assert got == hard_lines and len(hard_lines) >= NCH * 4
    assert (tmp_path / "soft.groups").read_text().splitlines() == soft_lines
    radio, soft_radio = (tmp_path / "quad.radio").read_text(), (tmp_path / "soft.radio").read_text()
    for c in range(NCH):
        s, k, q = hard[c].stats(), model_calls[c][1].stats(), model_calls[c][2]
        assert f"ch {c}: PI: {0x1000 + c:04X}\n" in radio, radio
        assert f"ch {c}: blocks: good {s['good']} corrected {s['corrected']} bad {s['bad']} BLER" in radio, radio
        assert (f"ch {c}: clock: locked 1 phase {k['phase']} bits {k['bits']} moves {k['moves']} half_moves {k['half_moves']} "
                f"resets 0 level {k['level']}\n") in radio, radio
        line = (f"ch {c}: carrier: phase {q.phase_deg():.2f} coherence {q.coherence():.3f} windows {q.windows} "
                f"resets {q.resets}\n")
        assert line in radio and line in soft_radio, (line, radio)
        assert q.windows == NB * 2836 // cm.W and q.resets == 0 and q.coherence() > 0.9
        s = soft[c].stats()
        assert f"ch {c}: blocks: good {s['good']} corrected {s['corrected']} bad {s['bad']} BLER" in soft_radio, soft_radio
        assert f"ch {c}: soft: blocks {soft[c].soft_blocks} flips {soft[c].soft_flips}\n" in soft_radio, soft_radio
    assert radio.count(" carrier: ") == NCH and radio.count(" clock: ") == NCH and "soft:" not in radio
    assert "carrier:" not in (tmp_path / "trk.radio").read_text()
    # every other file is the run's without the option
    others = sorted(p.name.split(".", 1)[1] for p in tmp_path.glob("trk.*") if p.suffix not in (".groups", ".radio"))
    assert {"pcm", "rds", "meter", "status"} <= set(others), others
    for ext in others:
        want = (tmp_path / f"trk.{ext}").read_bytes()
        assert (tmp_path / f"quad.{ext}").read_bytes() == want and (tmp_path / f"soft.{ext}").read_bytes() == want, ext
    assert sorted(p.name.split(".", 1)[1] for p in tmp_path.glob("quad.*")) == sorted(others + ["groups", "radio"])
    assert (tmp_path / "quad.pcm").stat().st_size == NB * NCH * 2 * 1470 * 2
