"""Host check of the lane-pair PLL step's loop filter (sdr_pll.hip pll_step_split, pll.cpp:41-42).

Lanes 2k and 2k+1 of a pair each own one of the loop filter's two state words (even: phaseEst, odd:
integrator) and issue one multiply and one add for it; phaseEst' is then one add of the two lanes'
sums, each lane reading its partner's. tools/pllmath/validate_lf.cpp evaluates that form operation
for operation, both lanes modelled, against the reference's five operations and compares the
integrator, phaseEst and the phaseEst value each lane converts for trigArg bit for bit.

The shipped form has no fused step and no excluded input: the select that keeps phaseEst' on the even
lane and the integrator on the odd lane is exact, so a -0 integrator is carried like any other value
(the grid counts those inputs and the test requires them to be compared, not skipped).
"""
from __future__ import annotations

import json
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pair_loop_filter_matches_reference_bit_for_bit(tmp_path):
    exe = tmp_path / "validate_lf"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", str(ROOT / "tools/pllmath/validate_lf.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "10000000"], capture_output=True, text=True, timeout=120)
    res = json.loads(r.stdout)
    print(res)
    # 10^7 random (integ, ph, e) triples: magnitudes past both state ranges, |e| up to pi
    assert res["n"] >= 10_000_000 and res["mismatch"] == 0, res
    # every triple of +-0, the smallest and largest denormals, +-FLT_MIN, +-pi, the range bounds,
    # +-FLT_MAX, +-inf and NaN, at four bandwidths; the -0 integrator is among them and is compared
    assert res["specials"] == 4 * 31 ** 3 and res["special_mismatch"] == 0, res
    assert res["negzero_integ"] == 4 * 31 ** 2, res
    # ph + RN(Kp e) exactly on a rounding tie (both parities of the last kept bit, both signs), and
    # the second sum s1A + s1B on a tie as well
    assert res["ties"] >= 100 and res["ties_second_sum"] >= 100 and res["tie_mismatch"] == 0, res
    # each lane carrying its own word from step to step (-0 starts and runs of +-0 errors included)
    assert res["chain_steps"] >= 5_000_000 and res["chain_mismatch"] == 0, res
    assert r.returncode == 0
