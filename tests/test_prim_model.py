"""CPU: the integer model of sdr_cdr (tests/prim_model.py) against the oracle's cdr on the rows the GPU
test uses, and the oracle's manchester / differential wrappers chained over one reference RDS run, which
pins their argument order before a GPU test leans on them. No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import prim_model as pm
from conftest import channel_input


@pytest.mark.parametrize("sps,n", pm.CDR_CASES)
def test_cdr_model_equals_the_oracle_on_finite_rows(oracle, sps, n):
    x, kinds, want = pm.cdr_rows(sps, n)
    assert x.shape == (pm.CDR_NCH, n)
    if n >= 2 * sps:
        assert {"nan", "inf2", "range"} <= set(kinds)
    for r, finite in enumerate(pm.cdr_finite(kinds)):
        got = pm.cdr_model(sps, x[r])
        if finite:                       # the oracle's C is undefined on the other rows: not called
            assert got == oracle.cdr(sps, x[r]), (r, kinds[r])
        if r in want:
            assert got == want[r], (r, kinds[r])


def test_cdr_model_non_finite_rows():
    """The header's sentence on hand-made rows: INT32_MIN for NaN / Inf / out of range, 32-bit wrap."""
    nan, inf = np.nan, np.inf
    rows = [
        ([5, 1, 2,  nan, 1, 2], 3, 2),          # 5 + 2^31 < 0: column 0 loses, column 2 (4) beats column 1 (2)
        ([5, 1, 2,  5, 1, 2], 3, 0),
        ([inf, 1, 2,  inf, 1, 2], 3, 2),        # 2 * 2^31 wraps to 0
        ([inf, 1, 2,  inf, 1, 2,  1, 0, 0], 3, 2),
        ([inf, 1, 2,  -inf, 1, 2,  7, 0, 0], 3, 0),   # wraps to 0, then 7
        ([3e9, 9, 1,  1, -3e9, 1], 3, 2),
        ([nan, nan], 2, 0),                     # both sums INT32_MIN: nothing wins
        ([-2147483648.0, 1], 2, 1),             # in range, magnitude 2^31: negative as int32
        ([2147483520.0, 1], 2, 0),              # the largest f32 below 2^31
        ([-0.5, 0.99], 2, 0),
    ]
    for x, sps, want in rows:
        assert pm.cdr_model(sps, np.array(x, np.float32)) == want, x


def test_oracle_manchester_differential_chain(oracle, synth):
    """oracle.manchester + oracle.differential, fed the symbols each block of an oracle.Channel(0).rds()
    run returns and keeping block_count, {half_symbol, start} and last_bit as orc_rds_block does
    (decoding from block 6 on, block_count = the block's index), reproduce that run's bits."""
    nblocks = 10
    iq = channel_input(synth, 0, nblocks)
    ch = oracle.Channel(0)
    state, last = [0, 0], 0
    decoded = 0
    for b in range(nblocks):
        r = ch.rds(ch.frontend(iq[b]))
        if b <= 5:
            assert r["bits"] is None
            continue
        bits = oracle.manchester(r["symbols"], b, state)
        out, last = oracle.differential(bits, b, last)
        assert np.array_equal(out, r["bits"]), f"block {b}"
        c = ch.state
        assert (state[0], state[1], last) == (c.half_symbol, c.start, c.last_bit), f"block {b}"
        decoded += len(out)
    assert decoded > 100


def test_oracle_manchester_refuses_an_empty_row(oracle):
    with pytest.raises(ValueError):
        oracle.manchester(np.zeros(0, np.int32), 1, [0, 1])
    out, last = oracle.differential(np.zeros(0, np.int32), 1, 1)
    assert len(out) == 0 and last == 1
