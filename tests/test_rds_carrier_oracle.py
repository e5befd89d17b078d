"""CPU: the carrier-phase derotator's model (tests/rds_carrier_model.py) on the oracle's rds_clean and on the
quadrature branch built from the oracle's primitives (tests/rds_quad_model.py), for synthetic stations, judged
by the tracker's and the decoders' models against the very same models on rds_clean alone. Each condition is a
comparison between the two inputs, not a count fixed here; the counts, the phase found and the counts of a
constant rotation by -44.5 degrees are printed, and DESIGN.md section 4j holds those of 200 blocks. No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import rds_carrier_model as cm
import rds_model as rm
import rds_quad_model as qm
import rds_soft_model as sm

NB = 120
CONSTANT_DEG = -44.5
_CACHE: dict = {}
STRONG = (0, 0.85, 0.01)
WEAK = [(0, 0.02, 0.01), (2, 0.015, 0.01), (7, 0.03, 0.02)]


def _complete(groups) -> int:
    return sum(1 for g in groups if g[1] == 15)


def _paths(synth, oracle, ch: int, amplitude: float, noise: float, nblocks: int = NB):
    """{input: {"hard": (groups, model), "soft": (groups, model)}} for the inputs "clean" (rds_clean), "derot" (the
    derotator's rows) and "const" (a float rotation by CONSTANT_DEG), each through its own tracker model; and the
    derotator's model."""
    key = (ch, amplitude, noise, nblocks)
    if key not in _CACHE:
        src = synth.FMMultiplexSource(ch, iq_amplitude=amplitude, noise=noise)
        oc = oracle.Channel(0, True)
        qb = qm.QuadBranch(oracle, oc)
        car = cm.Channel()
        trk = {k: sm.TrackChannel() for k in ("clean", "derot", "const")}
        bits = {k: ([], []) for k in trk}
        c0, s0 = np.float32(np.cos(np.deg2rad(CONSTANT_DEG))), np.float32(np.sin(np.deg2rad(CONSTANT_DEG)))
        phases = []
        for _ in range(nblocks):
            r = oc.rds(oc.frontend(src.next_block()), intermediates=True)
            xi = r["rds_clean"]
            xq = qb.block(r["rds_band"], r["gen_pilot"])["rds_clean_q"]
            rows = {"clean": xi, "derot": car.call(xi, xq), "const": xi * c0 + xq * s0}
            phases.append(car.phase_deg())
            for k, x in rows.items():
                _, b, s = trk[k].call(x)
                bits[k][0].extend(b)
                bits[k][1].extend(s)
        res = {k: {"hard": rm.decode(b), "soft": sm.decode(b, s, soft_bits=6)} for k, (b, s) in bits.items()}
        for k, both in res.items():
            for kind, (groups, st) in both.items():
                print(f"ch {ch} amplitude {amplitude} noise {noise} {k} {kind}: good {st.good} corrected {st.corrected} "
                      f"bad {st.bad} groups {len(groups)} complete {_complete(groups)}")
        tail = np.array(phases[nblocks // 4:])
        print(f"   carrier: phase {car.phase_deg():.2f} deg (mean {tail.mean():.2f}, sd {tail.std():.2f} over the last "
              f"{len(tail)} blocks), coherence {car.coherence():.3f}, windows {car.windows}, resets {car.resets}")
        _CACHE[key] = (res, car)
    return _CACHE[key]


def test_the_strong_station_loses_nothing(synth, oracle):
    res, car = _paths(synth, oracle, *STRONG)
    (cg, clean), (dg, derot) = res["clean"]["hard"], res["derot"]["hard"]
    assert derot.good >= clean.good and _complete(dg) >= _complete(cg)
    assert rm.station_ps(dg) == ({0x1000}, "MI355X00")
    (cs, _), (ds, dsoft) = res["clean"]["soft"], res["derot"]["soft"]
    assert _complete(ds) >= _complete(cs) and rm.station_ps(ds) == ({0x1000}, "MI355X00")
    assert car.resets == 0 and car.coherence() > 0.9


@pytest.mark.parametrize("ch,amplitude,noise", WEAK)
def test_a_weak_station_gains_blocks_and_groups(synth, oracle, ch, amplitude, noise):
    res, car = _paths(synth, oracle, ch, amplitude, noise)
    (cg, clean), (dg, derot) = res["clean"]["hard"], res["derot"]["hard"]
    assert derot.good > clean.good
    assert _complete(dg) > _complete(cg)
    (cs, _), (ds, _) = res["clean"]["soft"], res["derot"]["soft"]
    assert _complete(ds) >= _complete(cs)
    assert car.resets == 0
