"""CPU: what the receiver engine's five entry points (include/sdr_multi*.h) and the two file scans
(include/sdr_scan_run.h, include/sdr_wide_scan.h) refuse before anything starts. No case reaches a HIP
call: each returns SDR_E_INVALID on a machine without a GPU, where the first device call of an accepted
run would end the process."""
from __future__ import annotations

import ctypes as C

import pytest

from conftest import ROOT

INVALID = -1                                    # SDR_E_INVALID (include/sdr_amd.h)
vp = C.c_void_p
I32 = C.POINTER(C.c_int32)


class Opts(C.Structure):                        # sdr_multi_opts (include/sdr_multi.h)
    _fields_ = [("nch", C.c_int), ("mode", C.c_int), ("flags", C.c_int), ("device", C.c_int), ("pll_cus", C.c_int),
                ("in_path", C.c_char_p), ("d_iq", vp), ("row_stride", C.c_size_t), ("block_stride", C.c_size_t),
                ("nblocks", C.c_int), ("out_prefix", C.c_char_p), ("ncap", C.c_int), ("cap_blocks", C.c_int),
                ("cap_ch", vp), ("cap_lr", vp), ("cap_nbits", vp), ("cap_bits", vp), ("stamp_blocks", C.c_int),
                ("pll_end", vp)]


class Tuning(C.Structure):                      # sdr_multi_tuning (include/sdr_multi_tuned.h)
    _fields_ = [("nsrc", C.c_int), ("src", I32), ("khz", I32)]


class Wide(C.Structure):                        # sdr_multi_wide (include/sdr_multi_wide.h)
    _fields_ = [("W", C.c_int), ("nwide", C.c_int), ("shift", C.c_int), ("clips", vp)]


def scan_structs(pkg):
    class ScanRunOpts(C.Structure):             # sdr_scan_run_opts (include/sdr_scan_run.h)
        _fields_ = [("nrows", C.c_int), ("mode", C.c_int), ("device", C.c_int), ("in_path", C.c_char_p),
                    ("out_path", C.c_char_p), ("max_blocks", C.c_int), ("pick", pkg.ScanOpts),
                    ("max_stations", C.c_int), ("src", I32), ("khz", I32)]

    class ScanRunStats(C.Structure):
        _fields_ = [("stations", C.c_int), ("blocks", C.c_longlong), ("segments", C.c_longlong),
                    ("error", C.c_char * 256)]

    class WideScanOpts(C.Structure):            # sdr_wide_scan_opts (include/sdr_wide_scan.h)
        _fields_ = [("nwide", C.c_int), ("W", C.c_int), ("shift", C.c_int), ("mode", C.c_int), ("device", C.c_int),
                    ("in_path", C.c_char_p), ("out_path", C.c_char_p), ("max_blocks", C.c_int), ("pick", pkg.ScanOpts),
                    ("max_stations", C.c_int), ("src", I32), ("khz", I32)]

    class WideScanStats(C.Structure):
        _fields_ = [("stations", C.c_int), ("blocks", C.c_longlong), ("segments", C.c_longlong),
                    ("clips", C.c_longlong), ("error", C.c_char * 256)]
    return ScanRunOpts, ScanRunStats, WideScanOpts, WideScanStats


@pytest.fixture(scope="module")
def host(pkg):
    pkg.lib()
    h = C.CDLL(str(ROOT / "real-time-sdr_amd" / "libsdr_host.so"))
    h.sdr_multi_run.argtypes = [vp, vp]
    h.sdr_multi_run_tuned.argtypes = [vp, vp, vp]
    h.sdr_multi_run_metered.argtypes = [vp, vp, vp, vp]
    h.sdr_multi_run_finished.argtypes = [vp, vp, vp, vp, C.c_int, vp]
    h.sdr_multi_run_wide.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp]
    h.sdr_scan_run.argtypes = [vp, vp]
    h.sdr_wide_scan_run.argtypes = [vp, vp]
    return h


NCH = 3
MISSING = b"/nonexistent/sdr_multi_refusals.u8"    # never opened: every case is refused before the input is


def file_opts(**kw):
    """Options that pass the engine's own checks (a file input, NCH channels) but for what kw changes."""
    f = dict(nch=NCH, mode=0, pll_cus=16, in_path=MISSING)
    f.update(kw)
    return Opts(**f)


def tuning(nsrc=1, src=(0, 0, 0), khz=(0, 100, -100)):
    return Tuning(nsrc, (C.c_int32 * len(src))(*src), (C.c_int32 * len(khz))(*khz))


def entries(host, pkg):
    """Every entry point as f(opts) with otherwise acceptable arguments; opts is a pointer or None."""
    mo, ao, t, w = pkg.meter_opts(), pkg.audio_opts(), tuning(), Wide(4, 1, 0, None)
    ref = C.byref
    return {
        "run": lambda o: host.sdr_multi_run(o, None),
        "tuned": lambda o: host.sdr_multi_run_tuned(o, ref(t), None),
        "untuned": lambda o: host.sdr_multi_run_tuned(o, None, None),
        "metered": lambda o: host.sdr_multi_run_metered(o, None, ref(mo), None),
        "finished": lambda o: host.sdr_multi_run_finished(o, None, ref(mo), ref(ao), 1, None),
        "wide": lambda o: host.sdr_multi_run_wide(o, ref(w), ref(t), ref(mo), ref(ao), 1, None),
        "wide_null": lambda o: host.sdr_multi_run_wide(o, None, None, ref(mo), ref(ao), 1, None),
    }


def test_every_entry_refuses_bad_options(host, pkg):
    for name, f in entries(host, pkg).items():
        assert f(None) == INVALID, name                                        # NULL opts
        for nch in (0, -2):
            o = file_opts(nch=nch)
            assert f(C.byref(o)) == INVALID, (name, nch)
        o = file_opts(in_path=None)                                            # neither in_path nor d_iq
        assert f(C.byref(o)) == INVALID, name
        o = file_opts(in_path=None, row_stride=1 << 20, block_stride=1 << 22, nblocks=4)
        assert f(C.byref(o)) == INVALID, name                                  # strides but no d_iq
        o = file_opts(in_path=None, d_iq=1 << 20, row_stride=1 << 20, block_stride=1 << 22, nblocks=0)
        assert f(C.byref(o)) == INVALID, name                                  # a device input of no blocks


def test_tuned_refuses_a_bad_tuning(host, pkg):
    o, mo, ao = file_opts(), pkg.meter_opts(), pkg.audio_opts()
    N = pkg.tuner_table(0).shape[0]
    assert N == 2400
    none = C.cast(None, I32)
    good = tuning()
    bad = {
        "nsrc 0": tuning(nsrc=0),
        "nsrc -1": tuning(nsrc=-1),
        "nsrc > nch": tuning(nsrc=NCH + 1),
        "null src": Tuning(1, none, good.khz),
        "null khz": Tuning(1, good.src, none),
        "src = nsrc": tuning(nsrc=2, src=(0, 2, 1)),
        "src < 0": tuning(src=(0, -1, 0)),
        "src of the last channel": tuning(src=(0, 0, 1)),
        "khz > N/2": tuning(khz=(0, 0, N // 2 + 1)),
        "khz = -N/2": tuning(khz=(-N // 2, 0, 0)),
        "khz far off": tuning(khz=(0, 1 << 30, 0)),
    }
    for what, t in bad.items():
        p = C.byref(t)
        assert host.sdr_multi_run_tuned(C.byref(o), p, None) == INVALID, what
        assert host.sdr_multi_run_metered(C.byref(o), p, C.byref(mo), None) == INVALID, what
        assert host.sdr_multi_run_finished(C.byref(o), p, C.byref(mo), C.byref(ao), 0, None) == INVALID, what
        assert host.sdr_multi_run_wide(C.byref(o), None, p, None, C.byref(ao), 0, None) == INVALID, what
    bad_mode = file_opts(mode=4)                   # the tuning's bounds come from the mode's table
    assert host.sdr_multi_run_tuned(C.byref(bad_mode), C.byref(good), None) == INVALID


def test_metered_refuses_no_meter_options(host):
    o, t = file_opts(), tuning()
    assert host.sdr_multi_run_metered(C.byref(o), None, None, None) == INVALID
    assert host.sdr_multi_run_metered(C.byref(o), C.byref(t), None, None) == INVALID


def bad_audio_opts(pkg):
    """What sdr_audio_coeffs and the blend corners refuse (the engine takes any tau in [0, 1000] us; that
    only 0, 50 and 75 are offered is the CLI's rule)."""
    return {
        "tau 1001": pkg.audio_opts(tau_us=1001.0),
        "tau -5": pkg.audio_opts(tau_us=-5.0),
        "tau nan": pkg.audio_opts(tau_us=float("nan")),
        "hi = lo": pkg.audio_opts(blend_lo=1.0, blend_hi=1.0),
        "hi < lo": pkg.audio_opts(blend_lo=1.0, blend_hi=0.5),
        "hi nan": pkg.audio_opts(blend_hi=float("nan")),
    }


def test_finished_refuses(host, pkg):
    o, t, mo, ao = file_opts(), tuning(), pkg.meter_opts(), pkg.audio_opts()
    fn = host.sdr_multi_run_finished
    for tp in (None, C.byref(t)):
        assert fn(C.byref(o), tp, C.byref(mo), None, 0, None) == INVALID              # no audio options
        assert fn(C.byref(o), tp, None, None, 0, None) == INVALID
        assert fn(C.byref(o), tp, None, C.byref(ao), 1, None) == INVALID              # blend without a meter
        for what, bad in bad_audio_opts(pkg).items():
            for blend, mp in ((0, None), (0, C.byref(mo)), (1, C.byref(mo))):
                assert fn(C.byref(o), tp, mp, C.byref(bad), blend, None) == INVALID, (what, blend)
    # wide == NULL is exactly sdr_multi_run_finished
    fw = host.sdr_multi_run_wide
    assert fw(C.byref(o), None, None, C.byref(mo), None, 0, None) == INVALID
    assert fw(C.byref(o), None, None, None, C.byref(ao), 1, None) == INVALID
    for what, bad in bad_audio_opts(pkg).items():
        assert fw(C.byref(o), None, None, C.byref(mo), C.byref(bad), 1, None) == INVALID, what


def test_wide_refuses(host, pkg):
    L = pkg.lib()
    o, t, mo, ao = file_opts(), tuning(), pkg.meter_opts(), pkg.audio_opts()
    fw = host.sdr_multi_run_wide
    ref = C.byref

    def run(opts=o, wide=None, tune=t, mop=mo, aop=ao, blend=0):
        wide = wide if wide is not None else Wide(4, 1, 0, None)
        return fw(ref(opts), ref(wide), ref(tune) if tune is not None else None, ref(mop) if mop is not None else None,
                  ref(aop) if aop is not None else None, blend, None)

    assert run(tune=None) == INVALID                                           # a wide run is always tuned
    assert run(tune=None, mop=None, aop=None) == INVALID
    for what, w in {"nwide 0": Wide(4, 0, 0, None), "nwide -1": Wide(4, -1, 0, None), "nwide 4097": Wide(4, 4097, 0, None),
                    "shift 25": Wide(4, 1, 25, None), "W 5": Wide(5, 1, 0, None), "W 0": Wide(0, 1, 0, None)}.items():
        assert run(wide=w) == INVALID, what
        assert run(wide=w, mop=None, aop=None) == INVALID, what
    # nsrc within nch but beyond the rows the wide streams give: nwide * (2 W - 1) = 7
    nch = 8
    big = file_opts(nch=nch)
    t8 = tuning(nsrc=8, src=tuple(range(8)), khz=(0,) * 8)
    assert run(opts=big, tune=t8, wide=Wide(4, 1, 0, None)) == INVALID
    assert run(opts=big, tune=t8, wide=Wide(4, 1, 0, None), mop=None, aop=None) == INVALID
    assert run(tune=tuning(nsrc=NCH + 1)) == INVALID                           # the tuner's own bound
    assert run(tune=tuning(src=(0, 1, 0))) == INVALID
    # blend needs the meter and the finishing stage
    assert run(mop=None, blend=1) == INVALID
    assert run(aop=None, blend=1) == INVALID
    assert run(mop=None, aop=None, blend=1) == INVALID
    for what, bad in bad_audio_opts(pkg).items():
        assert run(aop=bad) == INVALID, what
        assert run(aop=bad, blend=1) == INVALID, what
    # device input: 4-byte aligned address and strides, rows no shorter than a wide row
    wide_iq = C.c_int()
    assert L.sdr_split_geometry(0, 4, None, None, C.byref(wide_iq), None, None) == 0
    row = 2 * wide_iq.value
    assert row % 4 == 0
    dev = dict(in_path=None, d_iq=1 << 20, row_stride=row, block_stride=row, nblocks=2)
    for what, kw in {"row_stride + 2": dict(row_stride=row + 2), "row_stride + 1": dict(row_stride=row + 1),
                     "block_stride + 2": dict(block_stride=row + 2), "d_iq + 2": dict(d_iq=(1 << 20) + 2),
                     "d_iq + 1": dict(d_iq=(1 << 20) + 1), "short rows": dict(row_stride=row - 4),
                     "no rows": dict(row_stride=0)}.items():
        od = file_opts(**{**dev, **kw})
        assert run(opts=od) == INVALID, what
        assert run(opts=od, mop=None, aop=None) == INVALID, what


def test_scan_run_refuses(host, pkg, tmp_path):
    SO, SS, _, _ = scan_structs(pkg)
    fn = host.sdr_scan_run
    pick = pkg.scan_opts()
    assert fn(None, None) == INVALID
    o = SO(nrows=1, in_path=MISSING, pick=pick)
    assert fn(C.byref(o), None) == INVALID

    def refused(opts, text):
        st = SS(stations=7, blocks=7, segments=7, error=b"stale")
        assert fn(C.byref(opts) if opts is not None else None, C.byref(st)) == INVALID, text
        assert st.error.decode() == text
        assert (st.stations, st.blocks, st.segments) == (0, 0, 0)

    needs = "scan: needs an input and nrows >= 1"
    refused(None, needs)
    refused(SO(nrows=1, in_path=None, pick=pick), needs)
    refused(SO(nrows=0, in_path=MISSING, pick=pick), needs)
    refused(SO(nrows=-3, in_path=MISSING, pick=pick), needs)
    arr = (C.c_int32 * 4)()
    none = C.cast(None, I32)
    refused(SO(nrows=1, in_path=MISSING, pick=pick, max_stations=4, src=none, khz=arr), "scan: null station arrays")
    refused(SO(nrows=1, in_path=MISSING, pick=pick, max_stations=4, src=arr, khz=none), "scan: null station arrays")
    missing = tmp_path / "no_such_capture.u8"
    refused(SO(nrows=1, in_path=str(missing).encode(), pick=pick), f"scan: cannot open {missing}")
    refused(SO(nrows=2, in_path=str(missing).encode(), pick=pick, max_stations=4, src=arr, khz=arr),
            f"scan: cannot open {missing}")
    # (the plain scan leaves step_khz to sdr_scan_pick: not refused before the input is opened)
    refused(SO(nrows=1, in_path=str(missing).encode(), pick=pkg.scan_opts(step_khz=0)), f"scan: cannot open {missing}")
    st = SS()
    bad_mode = SO(nrows=1, mode=4, in_path=str(missing).encode(), pick=pick)
    assert fn(C.byref(bad_mode), C.byref(st)) == INVALID and st.error.startswith(b"scan: ") and b"mode" in st.error


def test_wide_scan_run_refuses(host, pkg, tmp_path):
    _, _, WO, WS = scan_structs(pkg)
    fn = host.sdr_wide_scan_run
    pick = pkg.scan_opts()
    assert fn(None, None) == INVALID
    o = WO(nwide=1, W=4, in_path=MISSING, pick=pick)
    assert fn(C.byref(o), None) == INVALID

    def refused(opts, text):
        st = WS(stations=7, blocks=7, segments=7, clips=7, error=b"stale")
        assert fn(C.byref(opts) if opts is not None else None, C.byref(st)) == INVALID, text
        if text is not None:
            assert st.error.decode() == text
        assert (st.stations, st.blocks, st.segments, st.clips) == (0, 0, 0, 0)
        return st.error.decode()

    needs = "wide scan: needs an input and nwide >= 1"
    refused(None, needs)
    refused(WO(nwide=1, W=4, in_path=None, pick=pick), needs)
    refused(WO(nwide=0, W=4, in_path=MISSING, pick=pick), needs)
    refused(WO(nwide=-1, W=4, in_path=MISSING, pick=pick), needs)
    arr = (C.c_int32 * 4)()
    none = C.cast(None, I32)
    refused(WO(nwide=1, W=4, in_path=MISSING, pick=pick, max_stations=4, src=none, khz=arr), "wide scan: null station arrays")
    refused(WO(nwide=1, W=4, in_path=MISSING, pick=pick, max_stations=4, src=arr, khz=none), "wide scan: null station arrays")
    # before anything is opened: the path below does not exist, and the text is not "cannot open"
    missing = tmp_path / "no_such_capture.s8"
    path = str(missing).encode()
    for step in (0, -100):
        refused(WO(nwide=1, W=4, in_path=path, pick=pkg.scan_opts(step_khz=step)), "wide scan: step < 1")
    for W in (5, 0, 16):
        text = refused(WO(nwide=1, W=W, in_path=path, pick=pick), None)
        assert text.startswith("wide scan: ") and f"W {W} not 4, 8 or 10" in text, text
    text = refused(WO(nwide=1, W=4, mode=4, in_path=path, pick=pick), None)
    assert text.startswith("wide scan: ") and "mode" in text, text
    for W in (4, 8, 10):
        refused(WO(nwide=1, W=W, in_path=path, pick=pick), f"wide scan: cannot open {missing}")
    # behind the open and in front of every device call: the splitter's own argument rule, in its own words
    there = tmp_path / "short_capture.s8"
    there.write_bytes(bytes(16))
    path = str(there).encode()
    refused(WO(nwide=1, W=4, shift=25, in_path=path, pick=pick), "wide scan: split_create: shift 25 outside [1, 24]")
    refused(WO(nwide=4097, W=10, in_path=path, pick=pick), "wide scan: split_create: nwide 4097 outside [1, 4096]")
    refused(WO(nwide=4097, W=4, in_path=path, pick=pick), "wide scan: split_create: nwide 4097 outside [1, 4096]")
