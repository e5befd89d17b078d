"""CPU: the RDS symbol tracker's model (tests/rds_track_model.py) on the oracle's rds_clean of synthetic
stations, judged by the group decoder's model (tests/rds_model.py) against the reference bit path on the very
same input. Each condition is a comparison between the two paths, not a count fixed here; the counts are
printed, and DESIGN.md section 4h holds those of 200 blocks. No GPU."""
from __future__ import annotations

import pytest

import rds_model as rm
import rds_track_model as tm

NB = 120            # blocks of the inputs both paths read well; the weakest one runs 200
_CACHE: dict = {}


def _both_paths(synth, oracle, ch: int, amplitude: float, noise: float = 0.01, nblocks: int = NB):
    """{path: (groups, decoder model)} for path in ("ref", "trk"), and the tracker's model."""
    key = (ch, amplitude, noise, nblocks)
    if key not in _CACHE:
        src = synth.FMMultiplexSource(ch, iq_amplitude=amplitude, noise=noise)
        oc = oracle.Channel(0, True)
        trk = tm.Channel()
        ref_bits, trk_bits = [], []
        for _ in range(nblocks):
            r = oc.rds(oc.frontend(src.next_block()))
            if r["bits"] is not None:
                ref_bits += [int(v) for v in r["bits"]]
            trk_bits += trk.call(r["rds_clean"])[1]
        res = {"ref": rm.decode(ref_bits), "trk": rm.decode(trk_bits)}
        for name, (groups, st) in res.items():
            full = sum(1 for g in groups if g[1] == 15)
            print(f"ch {ch} amplitude {amplitude} noise {noise} {name}: good {st.good} corrected {st.corrected} bad {st.bad} "
                  f"slips {st.slips} acquired {st.acquired} lost {st.lost} groups {len(groups)} complete {full}")
        print(f"   tracker: {trk.stats()}")
        _CACHE[key] = (res, trk)
    return _CACHE[key]


@pytest.mark.parametrize("ch", [0, 3])
def test_the_fixture_channels_lose_their_slips(synth, oracle, ch):
    res, trk = _both_paths(synth, oracle, ch, 0.85)
    (_, ref), (groups, got) = res["ref"], res["trk"]
    assert got.slips == 0
    assert got.bad <= ref.bad and got.good >= ref.good
    assert rm.station_ps(groups) == ({0x1000 + ch}, f"MI355X{ch:02d}")
    assert trk.half_moves == 0 and trk.resets == 0 and trk.acquired == 1


def test_a_weak_station_gains_good_blocks(synth, oracle):
    res, _ = _both_paths(synth, oracle, 5, 0.03)
    ref, got = res["ref"][1], res["trk"][1]
    assert got.good > ref.good and got.slips == 0


def test_a_station_the_reference_path_cannot_read(synth, oracle):
    res, _ = _both_paths(synth, oracle, 2, 0.015, nblocks=200)
    (ref_groups, _), (groups, _) = res["ref"], res["trk"]
    complete = [g for g in groups if g[1] == 15 and g[0][0] == 0x1002]
    assert len(complete) >= 1
    assert len(ref_groups) <= len(groups)
