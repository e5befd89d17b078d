"""CPU: one rule per options record. The library's sdr_*_check functions (include/sdr_amd.h) hold the ranges
that the stages' creates and the receiver engine's validate() both go by; this walks every field of every
record over {lowest legal - 1, lowest legal, default, highest legal, highest legal + 1} (and a value of the
wrong stride or kind where the field has one), mode over -1..4 for the records a mode judges, and checks at
every point that
  - the check and the stage's create agree. Every create looks at nch before its options, so nch = 0 would
    hide them; the creates run instead with nch = 1 on device -1, which hipSetDevice -- the step behind the
    last option check of every create, in the code -- refuses: an accepted record gives SDR_E_HIP, a refused one
    SDR_E_INVALID with the check's text behind its own name. No device is touched;
  - the engine (sdr_multi_run_rds_carrier on an input path that does not exist) refuses what the check
    refuses. Accepted points are not tried: they would start a run.
And the sdr_last_error() text of every refusal in tests/golden/refusal_messages.json, recorded before the
stages shared these rules, is still what the library says."""
from __future__ import annotations

import ctypes as C
import importlib.util
import itertools
import json

import pytest

from conftest import ROOT
from test_multi_refusals import INVALID, NCH, Tuning, Wide, file_opts, tuning, vp
from test_multi_rds_refusals import Rds

OK, E_HIP = 0, -2
MODES = range(-1, 5)
GOLDEN = ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def host(pkg):
    pkg.lib()
    h = C.CDLL(str(ROOT / "real-time-sdr_amd" / "libsdr_host.so"))
    h.sdr_multi_run_rds_carrier.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    return h


def tail(text: bytes) -> str:
    """a refusal's text behind the name of who refused"""
    return text.decode().split(": ", 1)[-1]


def walk(defaults: dict, values: dict):
    """the defaults with one field at a time at each of its values"""
    for k, vs in values.items():
        for v in vs:
            yield {**defaults, k: v}


def agree(L, rc_check, rc_create, h, what):
    """the check's verdict and text against a create on device -1"""
    text = L.sdr_last_error()
    assert h.value is None, what
    if rc_check == OK:
        assert rc_create == E_HIP and text.startswith(b"hipSetDevice"), (what, rc_create, text)
    else:
        assert rc_check == INVALID == rc_create, (what, rc_check, rc_create)
    return text


def run_carrier(host, o=None, rds=None, track=None, soft=None, carrier=None, ao=None, tune=None, wide=None):
    """sdr_multi_run_rds_carrier on the tracker's clock, everything else acceptable"""
    ref = lambda x: C.byref(x) if x is not None else None
    o = o if o is not None else file_opts()
    rds = rds if rds is not None else Rds(2, 8)
    return host.sdr_multi_run_rds_carrier(ref(o), ref(wide), ref(tune), None, ref(ao), 0, ref(rds), 1, ref(track), ref(soft),
                                          ref(carrier), None)


def test_refusal_texts_are_the_recorded_ones(pkg):
    spec = importlib.util.spec_from_file_location("make_refusal_messages", GOLDEN / "make_refusal_messages.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = json.loads((GOLDEN / "refusal_messages.json").read_text())["cases"]
    pkg.lib()
    got = gen.record(C.CDLL(str(pkg.LIB_PATH)))     # the same library, without the package's prototypes
    assert list(got) == list(want)
    for name in want:
        assert got[name] == want[name], name
    assert len(want) > 150


def test_checks_refuse_null(pkg):
    L = pkg.lib()
    assert L.sdr_rds_opts_check(None) == INVALID and L.sdr_rds_soft_opts_check(None) == INVALID
    for mode in MODES:
        assert L.sdr_rds_track_opts_check(mode, None) == INVALID and L.sdr_rds_carrier_opts_check(mode, None) == INVALID
        assert L.sdr_audio_opts_check(mode, None) == INVALID
        assert L.sdr_tuner_check(mode, 1, 1, None, None) == INVALID
    assert L.sdr_version() == 3


RDS_VALUES = dict(max_burst=(-1, 0, 2, 5, 6), loss_blocks=(0, 1, 8, 64, 65))


def test_rds_opts(pkg, host):
    L, h = pkg.lib(), C.c_void_p()
    for f in walk(dict(max_burst=2, loss_blocks=8), RDS_VALUES):
        o = pkg.rds_opts(**f)
        rc = L.sdr_rds_opts_check(C.byref(o))
        said = L.sdr_last_error()
        text = agree(L, rc, L.sdr_rds_dec_create(C.byref(h), -1, 1, C.byref(o)), h, f)
        if rc != OK:
            assert tail(said) == tail(text) and text.startswith(b"rds_dec_create: "), f
            assert run_carrier(host, rds=Rds(f["max_burst"], f["loss_blocks"]), track=pkg.rds_track_opts()) == INVALID, f


def test_rds_soft_opts(pkg, host):
    L, h = pkg.lib(), C.c_void_p()
    for f in walk(dict(max_burst=2, loss_blocks=8, soft_bits=6), {**RDS_VALUES, "soft_bits": (-1, 0, 6, 7)}):
        o = pkg.rds_soft_opts(**f)
        rc = L.sdr_rds_soft_opts_check(C.byref(o))
        said = L.sdr_last_error()
        text = agree(L, rc, L.sdr_rds_dec_create_soft(C.byref(h), -1, 1, C.byref(o)), h, f)
        if rc != OK:
            assert tail(said) == tail(text), f
            assert run_carrier(host, track=pkg.rds_track_opts(), soft=o) == INVALID, f


def test_rds_track_opts(pkg, host):
    L, h = pkg.lib(), C.c_void_p()
    values = dict(qshift=(-1, 0, 10, 15, 16), acquire_bits=(0, 1, 32, 64, 65), half_bits=(15, 16, 40, 64, 65, 80))
    for mode, f in itertools.product(MODES, walk(dict(qshift=10, acquire_bits=32, half_bits=64), values)):
        o = pkg.rds_track_opts(**f)
        rc = L.sdr_rds_track_opts_check(mode, C.byref(o))
        said = L.sdr_last_error()
        text = agree(L, rc, L.sdr_rds_track_create(C.byref(h), -1, 1, mode, C.byref(o)), h, (mode, f))
        assert (rc == OK) == (mode == 0 and f["qshift"] in range(16) and f["acquire_bits"] in range(1, 65)
                              and f["half_bits"] in (16, 32, 48, 64)), (mode, f)
        if rc != OK:
            assert tail(said) == tail(text) and text.startswith(b"rds_track_create: "), (mode, f)
            assert run_carrier(host, o=file_opts(mode=mode), track=o) == INVALID, (mode, f)


def test_rds_carrier_opts(pkg, host):
    L, h = pkg.lib(), C.c_void_p()
    values = dict(qshift=(-1, 0, 10, 15, 16), avg_shift=(-1, 0, 3, 6, 7))
    for mode, f in itertools.product(MODES, walk(dict(qshift=10, avg_shift=3), values)):
        o = pkg.rds_carrier_opts(**f)
        rc = L.sdr_rds_carrier_opts_check(mode, C.byref(o))
        said = L.sdr_last_error()
        text = agree(L, rc, L.sdr_rds_carrier_create(C.byref(h), -1, 1, mode, C.byref(o)), h, (mode, f))
        assert (rc == OK) == (mode == 0 and f["qshift"] in range(16) and f["avg_shift"] in range(7)), (mode, f)
        if rc != OK:
            assert tail(said) == tail(text) and text.startswith(b"rds_carrier_create: "), (mode, f)
            assert run_carrier(host, o=file_opts(mode=mode), track=pkg.rds_track_opts(), carrier=o) == INVALID, (mode, f)


def test_audio_opts(pkg, host):
    L, h = pkg.lib(), C.c_void_p()
    nan, inf = float("nan"), float("inf")
    values = dict(tau_us=(-0.5, 0.0, 75.0, 1000.0, 1000.5, nan), blend_lo=(-inf, -1.0, 0.5, 1.999, 2.0, nan),
                  blend_hi=(0.5, 0.501, 2.0, 1e30, inf, nan))
    for mode, f in itertools.product(MODES, walk(dict(tau_us=75.0, blend_lo=0.5, blend_hi=2.0), values)):
        o = pkg.audio_opts(**f)
        rc = L.sdr_audio_opts_check(mode, C.byref(o))
        said = L.sdr_last_error()
        text = agree(L, rc, L.sdr_audio_create(C.byref(h), -1, 1, mode, 2, C.byref(o)), h, (mode, f))
        finite = all(abs(f[k]) < inf for k in ("blend_lo", "blend_hi"))      # (false for a NaN too)
        assert (rc == OK) == (mode in range(4) and 0.0 <= f["tau_us"] <= 1000.0 and finite
                              and f["blend_hi"] > f["blend_lo"]), (mode, f)
        if rc != OK:
            assert tail(said) == tail(text), (mode, f)
            assert run_carrier(host, o=file_opts(mode=mode), track=pkg.rds_track_opts(), ao=o) == INVALID, (mode, f)
    a, b = C.c_float(), C.c_float()
    assert L.sdr_audio_coeffs(0, 75.0, C.byref(a), C.byref(b)) == OK     # the rule the check holds is this one's
    assert L.sdr_audio_coeffs(0, 1000.5, C.byref(a), C.byref(b)) == INVALID


def test_split_check(pkg, host):
    L, h = pkg.lib(), C.c_void_p()
    values = dict(W=(3, 4, 5, 8, 10, 11), nwide=(0, 1, 4096, 4097), shift=(-1, 0, 1, 13, 24, 25))
    for mode, f in itertools.product(MODES, walk(dict(W=4, nwide=1, shift=0), values)):
        rc = L.sdr_split_check(mode, f["W"], f["nwide"], f["shift"])
        said = L.sdr_last_error()
        text = agree(L, rc, L.sdr_split_create(C.byref(h), -1, mode, f["W"], f["nwide"], f["shift"]), h, (mode, f))
        assert (rc == OK) == (mode in range(4) and f["W"] in (4, 8, 10) and 1 <= f["nwide"] <= 4096 and f["shift"] <= 24), \
            (mode, f)
        if rc != OK:
            assert tail(said) == tail(text) and text.startswith(b"split_create: "), (mode, f)
            w = Wide(f["W"], f["nwide"], f["shift"], None)
            assert run_carrier(host, o=file_opts(mode=mode), track=pkg.rds_track_opts(), tune=tuning(), wide=w) == INVALID, \
                (mode, f)


def test_tuner_check(pkg, host):
    """sdr_tuner_set takes a context, which a machine without a GPU cannot make: the check is held against the
    rule include/sdr_amd.h states (0 <= nsrc <= nch, nsrc = 0 untunes; 0 <= src < nsrc, -N/2 < khz <= N/2), and
    tests/test_gpu_stage_lifecycle.py holds sdr_tuner_set against the check on a context."""
    L = pkg.lib()
    none = C.cast(None, C.POINTER(C.c_int32))
    for mode in MODES:
        N = pkg.tuner_table(mode).shape[0] if mode in range(4) else 0
        half = N // 2
        cases = [dict(nsrc=n) for n in (-1, 0, 1, NCH, NCH + 1)]
        cases += [dict(nsrc=2, src=(0, s, 1)) for s in (-1, 0, 1, 2)] + [dict(nsrc=2, src=(0, 0, s)) for s in (-1, 1, 2)]
        cases += [dict(khz=(0, k, 0)) for k in (-half - 1, -half, -half + 1, 0, half, half + 1, 1 << 30, -(1 << 30))]
        cases += [dict(khz=(0, 0, k)) for k in (-half, half, half + 1)]
        for f in cases:
            t = tuning(**f)
            rc = L.sdr_tuner_check(mode, NCH, t.nsrc, t.src, t.khz)
            legal = mode in range(4) and 0 <= t.nsrc <= NCH and (t.nsrc == 0 or (
                all(0 <= t.src[c] < t.nsrc for c in range(NCH)) and all(-half < t.khz[c] <= half for c in range(NCH))))
            assert (rc == OK) == legal, (mode, f, L.sdr_last_error())
            if rc != OK:
                assert run_carrier(host, o=file_opts(mode=mode), track=pkg.rds_track_opts(), tune=t) == INVALID, (mode, f)
        for t in (Tuning(1, none, tuning().khz), Tuning(1, tuning().src, none)):
            assert L.sdr_tuner_check(mode, NCH, 1, t.src, t.khz) == INVALID
            assert run_carrier(host, o=file_opts(mode=mode), track=pkg.rds_track_opts(), tune=t) == INVALID
        assert L.sdr_tuner_check(mode, NCH, 0, none, none) == (OK if mode in range(4) else INVALID)   # untuned: no arrays
    # the engine's own rule: a tuned run has capture rows
    assert run_carrier(host, track=pkg.rds_track_opts(), tune=tuning(nsrc=0)) == INVALID
