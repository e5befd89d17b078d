"""Host check of the whole lane-pair PLL step and its chunk verdict (sdr_pll.hip pll_step_split,
pair_chunk) against the reference step evaluated with glibc (pll.cpp:36-50).

tools/pllmath/validate_step2.cpp models both lanes of a pair operation for operation, 16 steps per
chunk, and applies the kernel's acceptance rule: each lane's end of the e bracket, each lane's tie
key, |t| < 2^30 and the range of each lane's state word at the chunk's end. The rule has no test of
|e| (pll_math.h, "The cut at +-pi"): the validator evaluates the former |e| < pi - 2^-30 test beside
the rule and reports the accepted chunks it would have rejected ("e_range_only"); the special chunks
put the previous trigArg on and next to every k pi/2, |k| <= 8, with inputs of both signs, so that
base lands within 2^-22 of +-pi on either side of atan2's cut.

Criterion: no accepted chunk whose 16 phases or end state differ from the reference's bits.
"""
from __future__ import annotations

import json
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pair_step_accepts_only_the_reference_bits(tmp_path):
    exe = tmp_path / "validate_step2"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "real-time-sdr_amd/csrc"),
                    str(ROOT / "tools/pllmath/validate_step2.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "20000000"], capture_output=True, text=True, timeout=300)
    res = json.loads(r.stdout)
    print(res)
    assert res["poly"] == 0 and res["own"] == 0                       # the shipped evaluation order
    # 2 * 10^7 random steps; most chunks are accepted (the rest: invalid inputs, brackets, ties)
    assert res["steps"] >= 20_000_000 and res["accepted_steps"] >= 15_000_000, res
    assert res["wrong_steps"] == 0 and res["wrong_state"] == 0, res
    # both lanes always form the same e (Y = qA + qB commutes)
    assert res["lanes_disagree"] == 0, res
    # every kind of rejection occurred, so the rule was exercised, not bypassed
    assert all(res["rejected"][k] > 0 for k in ("e_bracket", "tie", "state")), res
    # the special chunks: trigArg next to k pi/2 and state words next to their bounds
    assert res["special_chunks"] >= 16_000 and res["special_accepted"] >= 8_000 and res["special_wrong"] == 0, res
    # accepted chunks with an e next to +-pi, which the former range test rejected: all the reference's bits
    assert res["special_e_range"] >= 500 and res["e_range_only"] >= 500 and res["e_range_only_wrong"] == 0, res
    assert r.returncode == 0
