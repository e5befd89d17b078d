"""GPU: the multi-channel receiver on a shared capture (include/sdr_multi_tuned.h; the CLI's --tune):
the 10-block composite of tests/tuner_model.py, one capture row per block, three stations. The
stereo PCM and RDS bits of every station equal the CPU model's, from a file through the CLI and from
device memory through sdr_multi_run_tuned in a child process, where a following untuned
sdr_multi_run on the engine's pooled contexts equals the oracle (the tuning does not leak)."""
from __future__ import annotations

import json
import subprocess
import sys

import numpy as np
import pytest

import tuner_model as tm
from conftest import ROOT, channel_input

pytestmark = pytest.mark.gpu

NB = tm.COMPOSITE_BLOCKS


def test_cli_tune_file_to_pcm(pkg, oracle, synth, tmp_path):
    exe = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"
    assert exe.exists(), "build with make"
    comp = tm.composite(synth)[0]
    comp.tofile(tmp_path / "in.u8")                           # [block][1 row][bytes]
    (tmp_path / "tune.txt").write_text("".join(f"0 {k}\n" for k in tm.COMPOSITE_KHZ))
    r = subprocess.run([str(exe), "3", "--tune", str(tmp_path / "tune.txt"), "--cus", "16", "--in",
                        str(tmp_path / "in.u8"), "--out", str(tmp_path / "rx")], capture_output=True, text=True,
                       timeout=180)
    assert r.returncode == 0, r.stderr
    assert "3 channels" in r.stderr and f"x {NB} blocks" in r.stderr and "PLLs persistent" in r.stderr, r.stderr
    assert "1 capture rows per block" in r.stderr, r.stderr
    model = tm.composite_model(pkg, oracle, synth)
    pcm = np.fromfile(tmp_path / "rx.pcm", np.int16).reshape(NB, 3, -1)
    for c in range(3):
        for b in range(NB):
            assert np.array_equal(pcm[b, c], model[c]["stereo"][b]), f"stereo station {c} block {b}"
    # a tune file with too few lines is refused before anything runs
    (tmp_path / "short.txt").write_text("0 0\n0 500\n")
    r = subprocess.run([str(exe), "3", "--tune", str(tmp_path / "short.txt"), "--in", str(tmp_path / "in.u8")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "3 lines" in r.stderr, r.stderr


def _check_bits(nbits, bits, ref_bits, what):
    if ref_bits is None:
        assert nbits == -1, "nbits " + what
    else:
        assert nbits == len(ref_bits), "nbits " + what
        assert np.array_equal(bits[:len(ref_bits)], ref_bits.astype(np.uint8)), "bits " + what


def test_run_tuned_device_input_and_pool(pkg, oracle, synth, tmp_path):
    comp = tm.composite(synth)[0][:, None, :]
    plain = np.stack([channel_input(synth, c, NB) for c in range(3)], axis=1)
    np.save(tmp_path / "comp.npy", np.ascontiguousarray(comp))
    np.save(tmp_path / "plain.npy", np.ascontiguousarray(plain))
    out = tmp_path / "cap.npz"
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "tuner_multi_child.py"), str(tmp_path / "comp.npy"),
                        str(tmp_path / "plain.npy"), str(out), "16"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    q = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert q["rc"] == [0, 0, -1], q                            # the out-of-range src is SDR_E_INVALID
    assert q["blocks"] == [NB, NB] and q["persistent"] == [1, 1], q
    got = np.load(out)
    model = tm.composite_model(pkg, oracle, synth)
    for c in range(3):
        for b in range(NB):
            w = f"station {c} block {b}"
            assert np.array_equal(got["lr1"][b, c], model[c]["stereo"][b]), "tuned stereo " + w
            _check_bits(got["nbits1"][b, c], got["bits1"][b, c], model[c]["bits"][b], "tuned " + w)
    for c in range(3):
        ref = oracle.run_channel(plain[:, c], 0, True)
        for b in range(NB):
            w = f"ch {c} block {b}"
            assert np.array_equal(got["lr2"][b, c], ref["stereo"][b]), "untuned run after the tuned one: stereo " + w
            _check_bits(got["nbits2"][b, c], got["bits2"][b, c], ref["bits"][b], "untuned " + w)
