"""GPU: the receiver engine's other paths (real-time-sdr_amd/host/sdr_multi_engine.cpp) give the bytes of
its default one. One input -- mode 0, 2 channels x 8 blocks from a file, the meter tests' synthetic
multiplex (8 blocks: the RDS decoding starts, rds.cpp:135, and every rotation slot of the consumers' LAG
is used more than once) -- through the CLI with --meter --deemph 75 --blend, so that every optional stage
runs. The baseline is the default run with --cus 16; each case is one more run, with another --cus or
with SDR_MULTI_* switches, and its five files equal the baseline's byte for byte."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

EXE = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"
NCH, NB = 2, 8
FILES = ("pcm", "rds", "meter", "audio", "status")


def _run(d, out, cus, env=None):
    assert EXE.exists(), "build with make"
    r = subprocess.run([str(EXE), str(NCH), "--cus", str(cus), "--in", str(d / "in.u8"), "--out", str(d / out),
                        "--meter", "--deemph", "75", "--blend"], capture_output=True, text=True, timeout=180,
                       env={**os.environ, **(env or {})})
    assert r.returncode == 0, r.stderr
    assert f"{NCH} channels x {NB} blocks" in r.stderr, r.stderr
    return r


@pytest.fixture(scope="module")
def base(synth, tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = tmp_path_factory.mktemp("paths")
    gen = synth.TorchMultiplexBatch(torch, NCH, 0, torch.device("cuda", 0), kinds=["normal", "no_pilot"], seed=11)
    np.stack([gen.next_block().cpu().numpy() for _ in range(NB)]).tofile(d / "in.u8")   # [block][channel][bytes]
    r = _run(d, "base", 16)
    assert "PLLs persistent" in r.stderr, r.stderr
    n_audio = 1470
    assert (d / "base.pcm").stat().st_size == (d / "base.audio").stat().st_size == NB * NCH * 2 * n_audio * 2
    assert (d / "base.meter").stat().st_size == NB * NCH * 64
    status = (d / "base.status").read_text().splitlines()
    assert len(status) == NCH and "STEREO" in status[0] and "STEREO" not in status[1], status
    assert (d / "base.pcm").read_bytes() != (d / "base.audio").read_bytes()
    return d


CASES = {
    "cus0": (0, {}, "per-block dispatch"),
    "edges0": (16, {"SDR_MULTI_EDGES": "0"}, "PLLs persistent"),
    "posts2": (16, {"SDR_MULTI_POSTS": "2"}, "PLLs persistent"),
    "fill0": (16, {"SDR_MULTI_FILL": "0"}, "PLLs persistent"),
    "nopools_fread": (16, {"SDR_MULTI_CTX_CACHE": "0", "SDR_MULTI_STREAM_CACHE": "0", "SDR_MULTI_PIN_CACHE": "0",
                           "SDR_MULTI_READERS": "1"}, "PLLs persistent"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_path_gives_the_default_bytes(base, case):
    cus, env, plls = CASES[case]
    r = _run(base, case, cus, env)
    assert plls in r.stderr, r.stderr
    for ext in FILES:
        assert (base / f"{case}.{ext}").read_bytes() == (base / f"base.{ext}").read_bytes(), ext
