"""GPU: the receiver and the scan on a wide capture through the CLI (include/sdr_multi_wide.h,
include/sdr_wide_scan.h; sdr_multi --wide): mode 0, W = 4, 3 blocks of one wide stream with three
stations within +-4.2 MHz, each within +-600 kHz of a row centre. `--wide 4 --scan` finds the three;
`--wide 4 --tune` on the wide file gives, byte for byte, the files of the existing `--tune` path on the
rows the model of tests/split_model.py splits off the same capture.

The tuner takes at most as many capture rows as it has channels (sdr_tuner_set: nsrc <= nch), so three
channels name rows 0..2: the stations sit in rows 0, 1 and 2 (centres -3600, -2400, -1200 kHz), and
rows.u8 holds those three of the model's seven rows per block, which is what `sdr_multi 3 --tune`
reads for a list whose largest row is 2."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import split_model as spm
from conftest import ROOT

pytestmark = pytest.mark.gpu

MODE, W, NB = 0, 4, 3
STATIONS_KHZ = (-3900, -2200, -1000)               # of the wide capture's centre
EXPECT = "0 -300\n1 200\n2 200\n"                  # src = row, khz off the row's centre
EXE = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"

_FILES: dict = {}


def _run(*args, timeout=180):
    return subprocess.run([str(EXE), *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout)


@pytest.fixture(scope="module")
def files(synth, tmp_path_factory):
    """wide.s8, rows.u8 and rx.stations, made once."""
    assert EXE.exists(), "build with make"
    d = tmp_path_factory.mktemp("wide")
    wide, clipped = spm.wide_composite(synth, W, NB, STATIONS_KHZ)
    assert clipped == 0
    rows, clips = spm.run(MODE, W, wide[:, None, :])
    _FILES["clips"] = clips[0]                                   # (gain 2 on three stations of 0.28 full scale: some clip)
    wide.tofile(d / "wide.s8")                                   # [block][1 stream][bytes]
    np.ascontiguousarray(rows[:, :3]).tofile(d / "rows.u8")      # [block][rows 0..2][bytes]
    return d


def test_cli_wide_scan(files):
    r = _run(1, "--wide", W, "--scan", "--in", files / "wide.s8", "--out", files / "rx")
    assert r.returncode == 0, r.stderr
    assert (files / "rx.stations").read_text() == EXPECT, r.stderr
    assert "3 stations in 1 wide streams x 7 rows" in r.stderr, r.stderr
    total = int(_FILES["clips"].sum())
    assert (f"splitter: {total} output components clipped" in r.stderr) == (total > 0), r.stderr


@pytest.mark.parametrize("extra,outs", [((), ("pcm", "rds")),
                                        (("--meter", "--deemph", "75", "--blend"), ("pcm", "rds", "meter", "audio", "status"))],
                         ids=["plain", "meter-deemph-blend"])
def test_cli_wide_tune_equals_rows_path(files, extra, outs):
    (files / "rx.stations").write_text(EXPECT)
    tag = "m" if extra else "p"
    a, b = files / f"a{tag}", files / f"b{tag}"
    ra = _run(3, "--tune", files / "rx.stations", "--cus", 16, "--in", files / "rows.u8", "--out", a, *extra)
    assert ra.returncode == 0, ra.stderr
    rb = _run(3, "--wide", W, "--tune", files / "rx.stations", "--cus", 16, "--in", files / "wide.s8", "--out", b, *extra)
    assert rb.returncode == 0, rb.stderr
    assert f"x {NB} blocks" in ra.stderr and f"x {NB} blocks" in rb.stderr, rb.stderr
    assert "from 1 wide streams x 7 rows per block" in rb.stderr, rb.stderr
    for r, n in enumerate(_FILES["clips"]):                      # the clip counters, exactly, where non-zero
        assert (f"wide stream 0 row {r}: {int(n)} output components clipped" in rb.stderr) == (n > 0), rb.stderr
    for ext in outs:
        fa, fb = a.with_suffix("." + ext).read_bytes(), b.with_suffix("." + ext).read_bytes()
        assert fa == fb, f".{ext} differs between the wide run and the run on the model's rows"
        assert len(fa) > 0 or ext == "rds"                       # (three blocks decode no RDS group yet)
    pcm = np.frombuffer(a.with_suffix(".pcm").read_bytes(), np.int16).reshape(NB, 3, -1)
    assert all(pcm[NB - 1, c].any() for c in range(3))           # the stations are received, not silence


def test_cli_wide_refusals(files):
    (files / "rx.stations").write_text(EXPECT)
    r = _run(3, "--wide", 5, "--tune", files / "rx.stations", "--in", files / "wide.s8", "--out", files / "x", timeout=60)
    assert r.returncode == 1 and "usage: sdr_multi" in r.stderr, r.stderr
    r = _run(3, "--wide", W, "--in", files / "wide.s8", "--out", files / "x", timeout=60)
    assert r.returncode == 1 and "usage: sdr_multi" in r.stderr, r.stderr
    (files / "row7.stations").write_text("0 -300\n1 200\n7 200\n")      # row 7 is no row of one wide stream
    r = _run(3, "--wide", W, "--tune", files / "row7.stations", "--in", files / "wide.s8", "--out", files / "x", timeout=60)
    assert r.returncode == 1, r.stderr
    assert not (files / "x.pcm").exists()
