"""GPU: the receiver engine's RF-metered runs (include/sdr_multi_meter.h; the CLI's --meter --rf). From device
memory through sdr_multi_run_metered in a child process, untuned and tuned, 3 channels, 4 blocks: PREFIX.rf equals
the CPU model's rows (tests/rf_model.py), PREFIX.rfstatus its lines, and every other file is byte for byte that of
the same run without SDR_FLAG_IF_ENVELOPE. The CLI writes the same two files from a file input."""
from __future__ import annotations

import json
import subprocess
import sys

import numpy as np
import pytest

import rf_model as rm
import tuner_model as tm
from conftest import ROOT, channel_input

pytestmark = pytest.mark.gpu

NB, NCH = 4, 3
TUNE = {"nsrc": 2, "src": [0, 0, 1], "khz": [-600, 500, 0]}
EXE = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"


@pytest.fixture(scope="module")
def inputs(synth):
    """plain u8 [NB][3][bytes]: two synthetic channels and a silent row; tuned u8 [NB][2][bytes]: the tuner tests'
    composite capture and a silent row."""
    plain = np.full((NB, NCH, 2 * synth.BLOCK_IQ), 128, np.uint8)
    for c in (0, 1):
        plain[:, c] = channel_input(synth, c, NB)
    tuned = np.full((NB, 2, 2 * synth.BLOCK_IQ), 128, np.uint8)
    tuned[:, 0] = tm.composite(synth)[0][:NB]
    return plain, tuned


@pytest.fixture(scope="module")
def model(pkg, oracle, inputs):
    """The model's rows [nch][NB] of both runs."""
    plain, tuned = inputs
    rows = {"plain_rf": []}
    for c in range(NCH):
        ch = rm.EnvChannel(oracle, 0)
        rows["plain_rf"].append([rm.rf_row(ch.block(plain[b, c])) for b in range(NB)])
    _, env = rm.run_tuned_env(pkg, oracle, 0, tuned, TUNE["src"], TUNE["khz"])
    rows["tuned_rf"] = [[rm.rf_row(e) for e in ce] for ce in env]
    return rows


@pytest.fixture(scope="module")
def child(inputs, tmp_path_factory):
    d = tmp_path_factory.mktemp("rf_multi")
    plain, tuned = inputs
    np.save(d / "plain.npy", plain)
    np.save(d / "tuned.npy", tuned)
    (d / "tune.json").write_text(json.dumps(TUNE))
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "rf_multi_child.py"), str(d / "plain.npy"),
                        str(d / "tuned.npy"), str(d / "tune.json"), str(d), "16"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    q = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    for name, res in q.items():
        assert res == {"rc": 0, "blocks": NB, "persistent": 1}, (name, res)
    return d


def _check_rf_files(d, name, rows):
    raw = (d / f"{name}.rf").read_bytes()
    assert len(raw) == NB * NCH * 32
    got = np.frombuffer(raw, rm.ROW_DTYPE).reshape(NB, NCH)
    for c in range(NCH):
        for b in range(NB):
            bad = rm.same_rows(got[b, c], rows[c][b])
            assert not bad, f"{name} ch {c} block {b}: {bad}\n got  {got[b, c]}\n want {rows[c][b]}"
    lines = (d / f"{name}.rfstatus").read_text().splitlines()
    assert lines == [rm.status_line(c, rm.run_long(rows[c])) for c in range(NCH)], lines
    return lines


@pytest.mark.parametrize("name", ["plain_rf", "tuned_rf"])
def test_run_metered_device_input(child, model, name):
    lines = _check_rf_files(child, name, model[name])
    assert lines[2] == "ch 2: level_dbfs -inf ripple 0.000 cnr_db -inf fade_db 0.000 crest_db 0.000 flags WEAK"   # silence
    assert lines[0].startswith("ch 0: level_dbfs -") and "inf" not in lines[0].split("cnr_db")[0]
    base = name[:-3]
    for ext in ("pcm", "rds", "meter", "status"):
        a, b = (child / f"{name}.{ext}").read_bytes(), (child / f"{base}.{ext}").read_bytes()
        assert a == b and (ext == "rds" or len(a) > 0), ext
    assert (child / f"{name}.pcm").stat().st_size == NB * NCH * 2 * 1470 * 2
    assert not (child / f"{base}.rf").exists() and not (child / f"{base}.rfstatus").exists()


def test_cli_meter_rf_from_a_file(child, inputs, tmp_path):
    """`sdr_multi 3 --meter --rf` on the same bytes from a file writes the device run's two files."""
    assert EXE.exists(), "build with make"
    inputs[0].tofile(tmp_path / "in.u8")
    r = subprocess.run([str(EXE), str(NCH), "--cus", "16", "--in", str(tmp_path / "in.u8"), "--out", str(tmp_path / "rx"),
                        "--meter", "--rf"], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    assert f"{NCH} channels" in r.stderr and "PLLs persistent" in r.stderr, r.stderr
    for ext in ("rf", "rfstatus", "pcm"):
        assert (tmp_path / f"rx.{ext}").read_bytes() == (child / f"plain_rf.{ext}").read_bytes(), ext
