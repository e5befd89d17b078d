"""CPU: what the 16-bit splitter's check and create, the receiver engine's sdr_multi_run_wide_fmt, the wide scan's
sdr_wide_scan_run_fmt (include/sdr_multi_wide16.h) and the CLI's --wide-format / --wide-gain refuse before anything
starts. No case reaches a device: creates run on device -1, the runs on an input that does not exist."""
from __future__ import annotations

import ctypes as C
import itertools
import subprocess

import pytest

from conftest import ROOT
from test_multi_refusals import INVALID, MISSING, NCH, Wide, file_opts, scan_structs, tuning, vp
from test_multi_rds_refusals import Rds
from test_opts_check import E_HIP, MODES, OK, agree, tail, walk

S8, S16, FIXED, AUTO = 0, 1, 0, 1
BIN = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"


class Fmt(C.Structure):                         # sdr_wide_fmt (include/sdr_multi_wide16.h)
    _fields_ = [("format", C.c_int), ("gain", C.c_int), ("target", C.c_int), ("shifts", C.POINTER(C.c_int)),
                ("shifts_out", C.POINTER(C.c_int)), ("peaks_out", C.POINTER(C.c_longlong))]


def table(*v):
    return (C.c_int * len(v))(*v)


@pytest.fixture(scope="module")
def host(pkg):
    pkg.lib()
    h = C.CDLL(str(ROOT / "real-time-sdr_amd" / "libsdr_host.so"))
    h.sdr_multi_run_wide_fmt.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp]
    h.sdr_multi_run_rds_carrier.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    h.sdr_wide_scan_run_fmt.argtypes = [vp, vp, vp]
    return h


def test_split16_check_is_create_s_rule(pkg, host):
    L, h = pkg.lib(), C.c_void_p()
    values = dict(W=(3, 4, 5, 8, 10, 11), nwide=(0, 1, 4096, 4097), shift=(-1, 0, 1, 22, 33, 34))
    for mode, f in itertools.product(MODES, walk(dict(W=4, nwide=1, shift=0), values)):
        rc = L.sdr_split16_check(mode, f["W"], f["nwide"], f["shift"])
        said = L.sdr_last_error()
        text = agree(L, rc, L.sdr_split16_create(C.byref(h), -1, mode, f["W"], f["nwide"], f["shift"]), h, (mode, f))
        assert (rc == OK) == (mode in range(4) and f["W"] in (4, 8, 10) and 1 <= f["nwide"] <= 4096 and f["shift"] <= 33), \
            (mode, f)
        if rc != OK:
            assert tail(said) == tail(text) and text.startswith(b"split16_create: "), (mode, f)
            w, t = Wide(f["W"], f["nwide"], f["shift"], None), tuning()
            fmt, o = Fmt(format=S16), file_opts(mode=mode)
            assert host.sdr_multi_run_wide_fmt(C.byref(o), C.byref(w), C.byref(t), None, None, 0, None, 0, None, None, None,
                                               C.byref(fmt), None) == INVALID, (mode, f)
    assert L.sdr_split16_create(None, -1, 0, 4, 1, 0) == INVALID
    assert E_HIP != INVALID


def test_engine_refuses(pkg, host):
    ref = lambda x: C.byref(x) if x is not None else None
    o, t = file_opts(), tuning()
    R = 7                                                                      # rows of W = 4

    def run(fmt, wide=Wide(4, 1, 0, None), tune=t, opts=o, rds=None, clock=0, track=None):
        return host.sdr_multi_run_wide_fmt(ref(opts), ref(wide), ref(tune), None, None, 0, ref(rds), clock, ref(track), None,
                                           None, ref(fmt), None)

    bad = {
        "format 2": Fmt(format=2), "format -1": Fmt(format=-1),
        "gain 2": Fmt(format=S16, gain=2), "gain -1": Fmt(format=S16, gain=-1),
        "target -1": Fmt(format=S16, gain=AUTO, target=-1), "target 128": Fmt(format=S16, gain=AUTO, target=128),
        "target 128, fixed": Fmt(format=S16, target=128),
        "auto and a table": Fmt(format=S16, gain=AUTO, shifts=table(*[22] * R)),
        "table with 0": Fmt(format=S16, shifts=table(*([22] * (R - 1) + [0]))),
        "table with 34": Fmt(format=S16, shifts=table(34, *[22] * (R - 1))),
    }
    for what, f in bad.items():
        assert run(f) == INVALID, what
        assert run(f, rds=Rds(2, 8), clock=1, track=pkg.rds_track_opts()) == INVALID, what
    good = Fmt(format=S16, gain=AUTO, target=90)
    assert run(good, wide=Wide(4, 1, 34, None)) == INVALID                     # the shift's range is the format's
    assert run(Fmt(format=S8), wide=Wide(4, 1, 25, None)) == INVALID           # ... 1..24 for s8, as ever
    assert run(None, wide=Wide(4, 1, 25, None)) == INVALID
    assert run(good, wide=None) == INVALID                                     # int16 rows are wide rows
    assert run(good, wide=None, tune=None) == INVALID
    assert run(good, tune=None) == INVALID                                     # and a wide run is always tuned
    assert run(good, opts=None) == INVALID
    assert run(good, tune=tuning(nsrc=0)) == INVALID
    # device input: rows no shorter than an int16 wide row
    wide_iq = C.c_int()
    assert pkg.lib().sdr_split_geometry(0, 4, None, None, C.byref(wide_iq), None, None) == 0
    row = 4 * wide_iq.value
    dev = dict(in_path=None, d_iq=1 << 20, row_stride=row, block_stride=row, nblocks=2)
    for what, kw in {"an s8 row": dict(row_stride=row // 2), "short rows": dict(row_stride=row - 4),
                     "row_stride + 2": dict(row_stride=row + 2), "d_iq + 2": dict(d_iq=(1 << 20) + 2)}.items():
        assert run(good, opts=file_opts(**{**dev, **kw})) == INVALID, what


def test_wide_scan_refuses(pkg, host, tmp_path):
    _, _, WO, WS = scan_structs(pkg)
    pick = pkg.scan_opts()
    missing = tmp_path / "no_such_capture.s16"
    path = str(missing).encode()

    def refused(opts, fmt, text):
        st = WS(stations=7, blocks=7, segments=7, clips=7, error=b"stale")
        assert host.sdr_wide_scan_run_fmt(C.byref(opts), C.byref(fmt) if fmt is not None else None, C.byref(st)) == INVALID, text
        assert text in st.error.decode(), (text, st.error)
        assert st.error.startswith(b"wide scan: ") and (st.stations, st.blocks, st.segments, st.clips) == (0, 0, 0, 0)

    o = WO(nwide=1, W=4, in_path=path, pick=pick)
    refused(o, Fmt(format=2), "format")
    refused(o, Fmt(format=S16, gain=2), "gain")
    refused(o, Fmt(format=S16, gain=AUTO, target=128), "target")
    refused(o, Fmt(format=S16, gain=AUTO, shifts=table(*[22] * 7)), "auto gain and a shifts table")
    refused(o, Fmt(format=S16, shifts=table(*[0] * 7)), "table")
    refused(WO(nwide=1, W=4, shift=34, in_path=path, pick=pick), Fmt(format=S16), "shift 34 outside [1, 33]")
    # an acceptable record gets as far as the input, like the s8 scan, and shift 25..33 is the format's to take
    for fmt in (Fmt(format=S16), Fmt(format=S16, gain=AUTO), Fmt(format=S16, gain=AUTO, target=127), None, Fmt(format=S8)):
        refused(o, fmt, f"cannot open {missing}")
    refused(WO(nwide=1, W=4, shift=33, in_path=path, pick=pick), Fmt(format=S16), f"cannot open {missing}")
    assert host.sdr_wide_scan_run_fmt(C.byref(o), None, None) == INVALID


def test_cli_usage_errors():
    """--wide-gain or --wide-format without --wide, a gain or a shift above 24 for the s8 splitter, a shift beside
    auto gain, and values outside their ranges end with the usage text, before any input is opened."""
    wide = ["--wide", "4", "--tune", "/nonexistent/stations", "--in", "/nonexistent/capture"]
    for args in (["--wide-format", "s16"], ["--wide-gain", "auto"], ["--wide-format", "s16", "--wide-gain", "auto"],
                 wide + ["--wide-gain", "auto"], wide + ["--wide-format", "s8", "--wide-gain", "auto"],
                 wide + ["--shift", "25"], wide + ["--wide-format", "s8", "--shift", "25"],
                 wide + ["--wide-format", "s16", "--shift", "34"], wide + ["--wide-format", "s16", "--shift", "0"],
                 wide + ["--wide-format", "s16", "--shift", "22", "--wide-gain", "auto"],
                 wide + ["--wide-format", "s24"], wide + ["--wide-format", "s16", "--wide-gain", "agc"],
                 wide + ["--wide-format", "s16", "--wide-gain", "auto:"], wide + ["--wide-format", "s16", "--wide-gain", "auto:0"],
                 wide + ["--wide-format", "s16", "--wide-gain", "auto:128"], wide + ["--wide-format", "s16", "--wide-gain", "auto:9x"],
                 wide + ["--wide-format"]):
        p = subprocess.run([str(BIN), "1"] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and p.stderr.startswith("usage: sdr_multi"), (args, p.stderr[:200])
    # accepted switches get as far as the tuning file
    for args in (wide + ["--wide-format", "s16"], wide + ["--wide-format", "s16", "--shift", "33"],
                 wide + ["--wide-format", "s16", "--wide-gain", "auto:127"], wide + ["--wide-format", "s8", "--shift", "24"]):
        p = subprocess.run([str(BIN), "1"] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and p.stderr.startswith("sdr_multi: cannot open /nonexistent/stations"), (args, p.stderr[:200])
