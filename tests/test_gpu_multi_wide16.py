"""GPU: the receiver and the scan on a 16-bit wide capture through the CLI (include/sdr_multi_wide16.h; sdr_multi
--wide W --wide-format s16), in the pattern of tests/test_gpu_multi_wide.py: mode 0, W = 4, 3 blocks of one wide
stream with three stations of unequal strength in rows 0, 1 and 2. `--tune` on the int16 file, with the fixed
default gain and with auto gain, gives byte for byte the files of the existing `--tune` path on the rows the model
of tests/split16_model.py splits off the same capture with the same shifts; PREFIX.wide holds the model's shifts,
peaks and clips; `--scan` finds the three."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import split16_model as s16
from conftest import ROOT

pytestmark = pytest.mark.gpu

MODE, W, NB = 0, 4, 3
R = 2 * W - 1
STATIONS_KHZ = (-3900, -2200, -1000)               # of the wide capture's centre
AMPS = (0.6, 0.2, 0.05)                            # of full scale: the default gain (2) clips the first, auto gain none
EXPECT = "0 -300\n1 200\n2 200\n"                  # src = row, khz off the row's centre
EXE = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"

_MODEL: dict = {}


def _run(*args, timeout=180):
    return subprocess.run([str(EXE), *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout)


@pytest.fixture(scope="module")
def files(synth, tmp_path_factory):
    """wide.s16, and per gain the model's rows 0..2 and its (shifts, peaks, clips), made once."""
    assert EXE.exists(), "build with make"
    d = tmp_path_factory.mktemp("wide16")
    wide, _w8, clipped = s16.wide_composite16(synth, W, NB, STATIONS_KHZ, AMPS)
    assert clipped == 0
    wide.tofile(d / "wide.s16")                                  # [block][1 stream][int16]
    acc = s16.sums(MODE, W, wide[:, None, :])
    fixed = np.full((1, R), s16.SHIFT_DEFAULT[W], np.int64)
    auto = s16.shifts_for(s16.finish_all(acc[:1], fixed)[2], 90, W)   # the rule on block 0's peaks
    auto60 = s16.shifts_for(s16.finish_all(acc[:1], fixed)[2], 60, W)
    for name, shifts in (("fixed", fixed), ("auto", auto), ("auto60", auto60), ("s20", np.full((1, R), 20, np.int64))):
        rows, clips, peaks = s16.finish_all(acc, shifts)
        np.ascontiguousarray(rows[:, :3]).tofile(d / f"rows_{name}.u8")
        _MODEL[name] = (shifts[0], peaks[0], clips[0])
    assert _MODEL["fixed"][2][0] > 0 and not _MODEL["auto"][2].any()   # the strong station clips at gain 2; auto: nothing
    assert (auto != fixed).any() and (auto60 != auto).any()
    return d


def _wide_file(path):
    return [tuple(int(v) for v in line.split()) for line in path.read_text().splitlines()]


CASES = [("fixed", (), ()), ("auto", ("--wide-gain", "auto"), ("--meter", "--deemph", "75", "--blend")),
         ("auto60", ("--wide-gain", "auto:60"), ()), ("s20", ("--shift", "20"), ())]


@pytest.mark.parametrize("name,gain,extra", CASES, ids=[c[0] for c in CASES])
def test_cli_wide16_tune_equals_rows_path(files, name, gain, extra):
    (files / "rx.stations").write_text(EXPECT)
    outs = ("pcm", "rds", "meter", "audio", "status") if extra else ("pcm", "rds")
    a, b = files / f"a_{name}", files / f"b_{name}"
    ra = _run(3, "--tune", files / "rx.stations", "--cus", 16, "--in", files / f"rows_{name}.u8", "--out", a, *extra)
    assert ra.returncode == 0, ra.stderr
    rb = _run(3, "--wide", W, "--wide-format", "s16", *gain, "--tune", files / "rx.stations", "--cus", 16,
              "--in", files / "wide.s16", "--out", b, *extra)
    assert rb.returncode == 0, rb.stderr
    assert f"x {NB} blocks" in ra.stderr and f"x {NB} blocks" in rb.stderr, rb.stderr
    assert "from 1 wide streams x 7 rows per block" in rb.stderr, rb.stderr
    shifts, peaks, clips = _MODEL[name]
    assert _wide_file(b.with_suffix(".wide")) == [(0, r, int(shifts[r]), int(peaks[r]), int(clips[r])) for r in range(R)]
    for r, n in enumerate(clips):                                # the clip counters, exactly, where non-zero
        assert (f"wide stream 0 row {r}: {int(n)} output components clipped" in rb.stderr) == (n > 0), rb.stderr
    for ext in outs:
        fa, fb = a.with_suffix("." + ext).read_bytes(), b.with_suffix("." + ext).read_bytes()
        assert fa == fb, f".{ext} differs between the wide run and the run on the model's rows"
        assert len(fa) > 0 or ext == "rds"                       # (three blocks decode no RDS group yet)
    assert not a.with_suffix(".wide").exists()                   # a run on capture rows writes none
    pcm = np.frombuffer(a.with_suffix(".pcm").read_bytes(), np.int16).reshape(NB, 3, -1)
    assert all(pcm[NB - 1, c].any() for c in range(3))           # the stations are received, not silence


@pytest.mark.parametrize("gain", [(), ("--wide-gain", "auto")], ids=["fixed", "auto"])
def test_cli_wide16_scan(files, gain):
    out = files / ("scan_auto" if gain else "scan_fixed")
    r = _run(1, "--wide", W, "--wide-format", "s16", *gain, "--scan", "--in", files / "wide.s16", "--out", out)
    assert r.returncode == 0, r.stderr
    assert out.with_suffix(".stations").read_text() == EXPECT, r.stderr
    assert "3 stations in 1 wide streams x 7 rows" in r.stderr, r.stderr
    total = int(_MODEL["auto" if gain else "fixed"][2].sum())
    assert (f"splitter: {total} output components clipped" in r.stderr) == (total > 0), r.stderr


def test_cli_wide16_usage_errors(files):
    (files / "rx.stations").write_text(EXPECT)
    base = (3, "--tune", files / "rx.stations", "--in", files / "wide.s16", "--out", files / "x")
    for args in (("--wide-format", "s16"), ("--wide-gain", "auto"), ("--wide", W, "--wide-gain", "auto"),
                 ("--wide", W, "--wide-format", "s16", "--shift", 34), ("--wide", W, "--shift", 25),
                 ("--wide", W, "--wide-format", "s16", "--shift", 22, "--wide-gain", "auto"),
                 ("--wide", W, "--wide-format", "s16", "--wide-gain", "auto:128")):
        r = _run(*base, *args, timeout=60)
        assert r.returncode == 1 and "usage: sdr_multi" in r.stderr, (args, r.stderr)
    assert not (files / "x.pcm").exists() and not (files / "x.wide").exists()
