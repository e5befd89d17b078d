#!/usr/bin/env python3
"""Golden fixture of the C ABI's refusal texts: for every create, call and bound of the stage handles that
libsdr_amd.so refuses before its first HIP call, the return code and the sdr_last_error() text.

record(L) runs the cases on a loaded library and returns {case: [code, text]}; tests/test_opts_check.py
compares a build's record with the fixture, byte for byte. No case reaches a HIP call: a refused create
stops at its checks, and a refused call stops before its handle is used, so zeroed memory stands in for one.
The texts hold numbers only, no addresses. Recorded from the library of the commit before the stage files
moved onto csrc/stage_host.h; the splitters' check, block, clips and 16-bit cases from the commit before
csrc/sdr_split16.hip moved into csrc/sdr_split.hip. Run it again only when a text is meant to change:
  python tests/golden/make_refusal_messages.py [path/to/libsdr_amd.so]
"""
from __future__ import annotations

import ctypes as C
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[2]
OUT = ROOT / "tests" / "golden" / "refusal_messages.json"
MAX_N = 19712                  # SDR_RDS_TRACK_MAX_N (include/sdr_amd.h)


def ints(*v):
    return (C.c_int * len(v))(*v)


def floats(*v):
    return (C.c_float * len(v))(*v)


def record(L: C.CDLL) -> dict[str, list]:
    L.sdr_last_error.restype = C.c_char_p
    out: dict[str, list] = {}
    sz, ref = C.c_size_t, C.byref

    def case(name, fn, *args):
        assert name not in out, name
        rc = getattr(L, fn)(*args)
        assert rc != 0, f"{name}: {fn} accepted what the fixture holds as refused"
        out[name] = [rc, L.sdr_last_error().decode()]

    h = C.c_void_p()
    # ---- creates: (out, device, ...); every refusal sits in front of hipSetDevice
    rds, soft, trk, car, aud = ints(2, 8), ints(2, 8, 6), ints(10, 32, 64), ints(10, 3), floats(75.0, 0.5, 2.0)
    case("rds_dec_create/out", "sdr_rds_dec_create", None, 0, 4, rds)
    case("rds_dec_create/opts", "sdr_rds_dec_create", ref(h), 0, 4, None)
    for nch in (0, -1):
        case(f"rds_dec_create/nch={nch}", "sdr_rds_dec_create", ref(h), 0, nch, rds)
    for o in ((-1, 8), (6, 8), (2, 0), (2, 65), (6, 0)):
        case(f"rds_dec_create/opts={o}", "sdr_rds_dec_create", ref(h), 0, 4, ints(*o))
    case("rds_dec_create_soft/out", "sdr_rds_dec_create_soft", None, 0, 4, soft)
    case("rds_dec_create_soft/opts", "sdr_rds_dec_create_soft", ref(h), 0, 4, None)
    case("rds_dec_create_soft/nch=0", "sdr_rds_dec_create_soft", ref(h), 0, 0, soft)
    for o in ((2, 8, -1), (2, 8, 7), (-1, 8, 6), (6, 8, 6), (2, 0, 6), (2, 65, 6), (6, 0, 7)):
        case(f"rds_dec_create_soft/opts={o}", "sdr_rds_dec_create_soft", ref(h), 0, 4, ints(*o))
    for name, good, bads in (("rds_track", trk, ((-1, 32, 64), (16, 32, 64), (10, 0, 64), (10, 65, 64), (10, 32, 0),
                                                 (10, 32, 8), (10, 32, 40), (10, 32, 80), (16, 0, 8))),
                             ("rds_carrier", car, ((-1, 3), (16, 3), (10, -1), (10, 7), (16, 7)))):
        fn = f"sdr_{name}_create"
        case(f"{name}_create/out", fn, None, 0, 4, 0, good)
        case(f"{name}_create/opts", fn, ref(h), 0, 4, 0, None)
        case(f"{name}_create/nch=0", fn, ref(h), 0, 0, 0, good)
        for mode in (-1, 1, 2, 3, 4):
            case(f"{name}_create/mode={mode}", fn, ref(h), 0, 4, mode, good)
        for o in bads:
            case(f"{name}_create/opts={o}", fn, ref(h), 0, 4, 0, ints(*o))
    case("audio_create/out", "sdr_audio_create", None, 0, 4, 0, 2, aud)
    case("audio_create/opts", "sdr_audio_create", ref(h), 0, 4, 0, 2, None)
    for mode in (-1, 4):
        case(f"audio_create/mode={mode}", "sdr_audio_create", ref(h), 0, 4, mode, 2, aud)
    case("audio_create/nch=0", "sdr_audio_create", ref(h), 0, 0, 0, 2, aud)
    case("audio_create/width=3", "sdr_audio_create", ref(h), 0, 4, 0, 3, aud)
    for o in ((-1.0, 0.5, 2.0), (1000.5, 0.5, 2.0), (float("nan"), 0.5, 2.0), (75.0, 2.0, 2.0), (75.0, 2.0, 0.5),
              (75.0, 0.5, float("inf")), (75.0, float("nan"), 2.0)):
        for mode in (0, 1, 2, 3):
            case(f"audio_create/mode={mode}/opts={o}", "sdr_audio_create", ref(h), 0, 4, mode, 2, floats(*o))
    case("meter_create/out", "sdr_meter_create", None, 0, 4, 0)
    case("meter_create/mode=4", "sdr_meter_create", ref(h), 0, 4, 4)
    case("meter_create/nch=0", "sdr_meter_create", ref(h), 0, 0, 0)
    case("scan_create/out", "sdr_scan_create", None, 0, 0, 1)
    for mode, nsrc in ((4, 1), (-1, 1), (0, 0), (0, 65536)):
        case(f"scan_create/mode={mode}/nsrc={nsrc}", "sdr_scan_create", ref(h), 0, mode, nsrc)
    case("split_create/out", "sdr_split_create", None, 0, 0, 4, 1, 0)
    for a in ((4, 4, 1, 0), (-1, 4, 1, 0), (0, 5, 1, 0), (0, 0, 1, 0), (0, 4, 0, 0), (0, 8, 4097, 0), (0, 10, 1, 25),
              (3, 4, 4096, 25)):
        case(f"split_create/mode,W,nwide,shift={a}", "sdr_split_create", ref(h), 0, *a)
    assert h.value is None
    case("tuner_set/ctx", "sdr_tuner_set", None, 1, None, None, None)

    # ---- the handles' other entries on NULL
    for name in ("rds_dec", "rds_track", "rds_carrier", "audio", "meter", "scan", "split"):
        case(f"{name}_destroy/null", f"sdr_{name}_destroy", None)
        case(f"{name}_reset/null", f"sdr_{name}_reset", None, None)
    buf = C.create_string_buffer(64)
    for fn in ("sdr_rds_stats_read", "sdr_rds_soft_stats_read", "sdr_rds_track_stats_read", "sdr_rds_carrier_stats_read",
               "sdr_meter_read", "sdr_audio_read_state"):
        case(f"{fn[4:]}/handle", fn, None, buf, None)

    # ---- calls: zeroed memory stands in for the handle, which no refusal looks into
    stand_in = C.create_string_buffer(256)
    vp = C.c_void_p                                   # (a bare int would be passed as a C int)
    off = lambda p, k: vp(p.value + k)
    t = vp(C.addressof(stand_in))
    for fn in ("sdr_rds_stats_read", "sdr_rds_soft_stats_read", "sdr_rds_track_stats_read", "sdr_rds_carrier_stats_read",
               "sdr_meter_read", "sdr_audio_read_state"):
        case(f"{fn[4:]}/host", fn, t, None, None)
    row, row2, orow = (C.c_float * 8)(), (C.c_float * 8)(), (C.c_float * 8)()
    nb, bits, sft = (C.c_int32 * 1)(), (C.c_uint8 * 256)(), (C.c_uint16 * 256)()
    x, q, y = vp(C.addressof(row)), vp(C.addressof(row2)), vp(C.addressof(orow))
    n_, b_, s_ = vp(C.addressof(nb)), vp(C.addressof(bits)), vp(C.addressof(sft))
    rot = lambda name, *a: case(f"rds_carrier_rotate/{name}", "sdr_rds_carrier_rotate", *a)
    rot("handle", None, x, sz(8), q, sz(8), 8, y, sz(8), None)
    rot("clean_i", t, None, sz(8), q, sz(8), 8, y, sz(8), None)
    rot("clean_q", t, x, sz(8), None, sz(8), 8, y, sz(8), None)
    rot("out", t, x, sz(8), q, sz(8), 8, None, sz(8), None)
    rot("n=-1", t, x, sz(8), q, sz(8), -1, y, sz(8), None)
    rot("n=max+1", t, x, sz(MAX_N + 1), q, sz(MAX_N + 1), MAX_N + 1, y, sz(MAX_N + 1), None)
    rot("stride_i", t, x, sz(7), q, sz(8), 8, y, sz(8), None)
    rot("stride_q", t, x, sz(8), q, sz(7), 8, y, sz(8), None)
    rot("out_stride", t, x, sz(8), q, sz(8), 8, y, sz(7), None)
    for name, a in (("clean_i", (off(x, 2), q, y)), ("clean_q", (x, off(q, 1), y)), ("out", (x, q, off(y, 3)))):
        rot(f"misaligned {name}", t, a[0], sz(8), a[1], sz(8), 4, a[2], sz(8), None)
    trkb = lambda name, *a: case(f"rds_track_bits/{name}", "sdr_rds_track_bits", *a)
    trkb("handle", None, x, sz(8), 8, n_, b_, sz(256), None)
    trkb("clean", t, None, sz(8), 8, n_, b_, sz(256), None)
    trkb("nbits", t, x, sz(8), 8, None, b_, sz(256), None)
    trkb("bits", t, x, sz(8), 8, n_, None, sz(256), None)
    trkb("n=-1", t, x, sz(8), -1, n_, b_, sz(256), None)
    trkb("n=max+1", t, x, sz(MAX_N + 1), MAX_N + 1, n_, b_, sz(256), None)
    trkb("clean_stride", t, x, sz(7), 8, n_, b_, sz(256), None)
    trkb("bits_stride", t, x, sz(8), 8, n_, b_, sz(255), None)
    trkb("misaligned clean", t, off(x, 2), sz(8), 4, n_, b_, sz(256), None)
    trks = lambda name, *a: case(f"rds_track_bits_soft/{name}", "sdr_rds_track_bits_soft", *a)
    trks("handle", None, x, sz(8), 8, n_, b_, sz(256), s_, sz(256), None)
    trks("soft", t, x, sz(8), 8, n_, b_, sz(256), None, sz(256), None)
    trks("soft_stride", t, x, sz(8), 8, n_, b_, sz(256), s_, sz(255), None)
    trks("misaligned soft", t, x, sz(8), 8, n_, b_, sz(256), off(s_, 1), sz(256), None)
    trks("n=-1", t, x, sz(8), -1, n_, b_, sz(256), s_, sz(256), None)
    trks("clean_stride", t, x, sz(7), 8, n_, b_, sz(256), s_, sz(256), None)
    trks("bits_stride", t, x, sz(8), 8, n_, b_, sz(255), s_, sz(256), None)
    grp = lambda name, *a: case(f"rds_groups/{name}", "sdr_rds_groups", *a)
    grp("handle", None, n_, b_, sz(256), None)
    grp("nbits", t, None, b_, sz(256), None)
    grp("bits", t, n_, None, sz(256), None)
    grp("bits_stride", t, n_, b_, sz(255), None)
    grs = lambda name, *a: case(f"rds_groups_soft/{name}", "sdr_rds_groups_soft", *a)
    grs("handle", None, n_, b_, sz(256), s_, sz(256), None)
    grs("soft", t, n_, b_, sz(256), None, sz(256), None)
    grs("bits_stride", t, n_, b_, sz(255), s_, sz(256), None)
    grs("soft_stride", t, n_, b_, sz(256), s_, sz(255), None)
    grs("misaligned soft", t, n_, b_, sz(256), off(s_, 1), sz(256), None)
    grs("hard handle", t, n_, b_, sz(256), s_, sz(256), None)      # zeroed: not a soft handle
    assert bytes(stand_in) == bytes(256) and nb[0] == 0

    # ---- the 16-bit splitter (recorded before it shared the 8-bit splitter's unit and argument rule)
    case("split16_create/out", "sdr_split16_create", None, 0, 0, 4, 1, 0)
    for a in ((4, 4, 1, 0), (-1, 4, 1, 0), (0, 5, 1, 0), (0, 0, 1, 0), (0, 4, 0, 0), (0, 8, 4097, 0), (0, 10, 1, 34),
              (3, 4, 4096, 34)):
        case(f"split16_create/mode,W,nwide,shift={a}", "sdr_split16_create", ref(h), 0, *a)
        case(f"split16_check/mode,W,nwide,shift={a}", "sdr_split16_check", *a)
    assert h.value is None
    ll = C.c_longlong
    for a in ((100, 90, 5), (100, 90, 0), (100, 0, 4), (100, 128, 8), (-1, 90, 10)):
        case(f"split16_shift_for/peak,target,W={a}", "sdr_split16_shift_for", ll(a[0]), a[1], a[2])
    case("split16_destroy/null", "sdr_split16_destroy", None)
    case("split16_reset/null", "sdr_split16_reset", None, None)
    case("split16_set_shifts/null", "sdr_split16_set_shifts", None, ints(24), None)
    case("split16_block/null", "sdr_split16_block", None, x, sz(8), y, sz(8), None)
    case("split16_clips/null", "sdr_split16_clips", None, x, None)
    case("split16_peaks/null", "sdr_split16_peaks", None, x, 0, None)
    # on the stand-in: null arguments, which stop in front of the handle, and strides and pointers that a block
    # of any size refuses (the texts hold W and block_iq of the handle, 0 of a zeroed one)
    case("split16_set_shifts/shifts", "sdr_split16_set_shifts", t, None, None)
    case("split16_block/wide", "sdr_split16_block", t, None, sz(8), y, sz(8), None)
    case("split16_block/rows", "sdr_split16_block", t, x, sz(8), None, sz(8), None)
    case("split16_block/wide_stride", "sdr_split16_block", t, x, sz(6), y, sz(8), None)
    case("split16_block/misaligned wide", "sdr_split16_block", t, off(x, 2), sz(8), y, sz(8), None)
    case("split16_block/row_stride", "sdr_split16_block", t, x, sz(8), y, sz(7), None)
    case("split16_block/misaligned rows", "sdr_split16_block", t, x, sz(8), off(y, 1), sz(8), None)
    case("split16_clips/clips", "sdr_split16_clips", t, None, None)
    case("split16_peaks/peaks", "sdr_split16_peaks", t, None, 0, None)
    # ---- the 8-bit splitter's cases that its shared rules now answer
    for a in ((4, 4, 1, 0), (-1, 4, 1, 0), (0, 5, 1, 0), (0, 0, 1, 0), (0, 4, 0, 0), (0, 8, 4097, 0), (0, 10, 1, 25),
              (3, 4, 4096, 25)):
        case(f"split_check/mode,W,nwide,shift={a}", "sdr_split_check", *a)
    case("split_block/null", "sdr_split_block", None, x, sz(8), y, sz(8), None)
    case("split_clips/null", "sdr_split_clips", None, x, None)
    case("split_block/wide", "sdr_split_block", t, None, sz(8), y, sz(8), None)
    case("split_block/rows", "sdr_split_block", t, x, sz(8), None, sz(8), None)
    case("split_block/wide_stride", "sdr_split_block", t, x, sz(6), y, sz(8), None)
    case("split_block/misaligned wide", "sdr_split_block", t, off(x, 2), sz(8), y, sz(8), None)
    case("split_block/row_stride", "sdr_split_block", t, x, sz(8), y, sz(7), None)
    case("split_block/misaligned rows", "sdr_split_block", t, x, sz(8), off(y, 1), sz(8), None)
    case("split_clips/clips", "sdr_split_clips", t, None, None)
    assert bytes(stand_in) == bytes(256)
    return out


def main() -> None:
    path = sys.argv[1] if len(sys.argv) > 1 else ROOT / "real-time-sdr_amd" / "libsdr_amd.so"
    rec = record(C.CDLL(str(path)))
    OUT.write_text(json.dumps({"source": "sdr_last_error() of every refused case of make_refusal_messages.record()",
                               "cases": rec}, indent=0) + "\n")
    print(f"wrote {OUT} ({len(rec)} cases)")


if __name__ == "__main__":
    main()
