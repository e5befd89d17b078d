"""CPU: the soft decisions' models (tests/rds_soft_model.py) on the oracle's rds_clean of synthetic stations
and on a stream without DSP, judged against the hard decoder's model (tests/rds_model.py) on the very same
tracked bits. Each condition is a comparison between the two decoders, not a count fixed here; the counts and
the wrong-PI counts are printed, and DESIGN.md section 4i holds them. No GPU."""
from __future__ import annotations

import pytest

import rds_model as rm
import rds_soft_model as sm

NB = 200
_CACHE: dict = {}


def _complete(groups) -> int:
    return sum(1 for g in groups if g[1] == 15)


def _wrong_pi(groups, pi: int) -> int:
    return sum(1 for g in groups if (g[1] & 1) and g[0][0] != pi)


def _report(name, pi, res):
    for kind, (groups, st) in res.items():
        print(f"{name} {kind}: good {st.good} corrected {st.corrected} bad {st.bad} slips {st.slips} acquired {st.acquired} "
              f"lost {st.lost} groups {len(groups)} complete {_complete(groups)} wrong PI {_wrong_pi(groups, pi)}"
              + (f" soft blocks {st.soft_blocks} flips {st.soft_flips}" if kind == "soft" else ""))


def _both(synth, oracle, ch: int, amplitude: float, noise: float = 0.01, nblocks: int = NB):
    """{"hard": (groups, model), "soft": (groups, model)} on the soft tracker model's bits of the oracle's rds_clean."""
    key = (ch, amplitude, noise, nblocks)
    if key not in _CACHE:
        src = synth.FMMultiplexSource(ch, iq_amplitude=amplitude, noise=noise)
        oc = oracle.Channel(0, True)
        trk = sm.TrackChannel()
        bits, soft = [], []
        for _ in range(nblocks):
            _, b, s = trk.call(oc.rds(oc.frontend(src.next_block()))["rds_clean"])
            bits += b
            soft += s
        res = {"hard": rm.decode(bits), "soft": sm.decode(bits, soft, soft_bits=6)}
        _report(f"ch {ch} amplitude {amplitude} noise {noise}", 0x1000 + ch, res)
        _CACHE[key] = res
    return _CACHE[key]


def test_a_strong_station_is_left_alone(synth, oracle):
    res = _both(synth, oracle, 0, 0.85)
    (hg, hard), (sg, soft) = res["hard"], res["soft"]
    assert sg == hg and soft.stats() == hard.stats()
    assert rm.station_ps(sg) == ({0x1000}, "MI355X00")


@pytest.mark.parametrize("ch,amplitude,noise", [(0, 0.02, 0.01), (2, 0.015, 0.01), (7, 0.03, 0.02)])
def test_a_weak_station_gains_groups(synth, oracle, ch, amplitude, noise):
    res = _both(synth, oracle, ch, amplitude, noise)
    (hg, hard), (sg, soft) = res["hard"], res["soft"]
    assert _complete(sg) > _complete(hg)
    assert soft.bad < hard.bad
    assert soft.lost <= hard.lost
    assert rm.station_ps(sg)[1] == f"MI355X{ch:02d}"
    assert soft.soft_blocks >= 1 and soft.soft_flips >= soft.soft_blocks


@pytest.mark.parametrize("seed", [1, 2])
def test_the_stream_without_dsp_gains_groups(synth, seed):
    clean = rm.make_streams(synth)[0]
    x = sm.noisy_chips(clean, seed)
    bits, soft, _ = sm.track_soft([x[k:k + 2836] for k in range(0, len(x), 2836)])
    res = {"hard": rm.decode(bits), "soft": sm.decode(bits, soft, soft_bits=6)}
    _report(f"chips at 300 under +-2500, seed {seed}", 0x2001, res)
    assert _complete(res["soft"][0]) > _complete(res["hard"][0])
    assert res["soft"][1].bad < res["hard"][1].bad
