"""Writes tests/golden/rds_groups_mode0.json: the group lines the model (tests/rds_model.py, default
options) gives for the 24 blocks of bits in golden_mode0.npz, channels 0 and 3, one call per block.
    python tests/golden/make_rds_groups.py"""
from __future__ import annotations

import json
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import rds_model as rm  # noqa: E402


def main():
    z = np.load(HERE / "golden_mode0.npz")
    out = {"mode": 0, "nblocks": 24, "options": rm.DEFAULTS, "channels": {}}
    for c in (0, 3):
        ch = rm.Channel()
        groups = []
        for blk in z[f"ch{c}_bits"]:
            s = str(blk)
            groups += ch.call(len(s) if s else -1, [int(x) for x in s])
        out["channels"][str(c)] = {"groups": [rm.group_line(c, g) for g in groups], "stats": ch.stats()}
    (HERE / "rds_groups_mode0.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
