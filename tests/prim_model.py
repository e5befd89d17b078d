"""Integer model of sdr_cdr as include/sdr_amd.h states it, and the rows the CPU and GPU tests of the
batched primitives share. numpy only.

cdr: offset i < sps sums the n // sps samples x[k * sps + i]. A sample is truncated toward zero to int32;
NaN, infinities and values outside int32 count as INT32_MIN. The sum of the magnitudes is 32 bits and
wraps. An offset wins only with a sum > 0 read as int32; the lowest offset wins among equal sums; 0 when
no offset wins. For finite in-range rows whose sums stay below 2^31 this is the reference's cdr()
(rds_utilities.cpp:4-21), whose C is undefined elsewhere."""
from __future__ import annotations

import numpy as np

CDR_CASES = [(1, 10), (2, 7), (39, 2836), (39, 38), (63, 635), (64, 2879), (64, 63)]
CDR_NCH = 67
CDR_KINDS = ("gauss", "zero", "subone", "tie", "last", "first", "big", "nan", "inf2", "range")


def cdr_model(sps: int, x) -> int:
    x = np.asarray(x, np.float32)
    nk = len(x) // sps
    if nk == 0:
        return 0
    a = x[:nk * sps].reshape(nk, sps).astype(np.float64)
    ok = (a >= -2147483648.0) & (a < 2147483648.0)            # False for NaN
    v = np.where(ok, np.trunc(np.where(ok, a, 0.0)), -2147483648.0).astype(np.int64)
    s = (np.abs(v).astype(np.uint64).sum(axis=0) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    best = int(s.max())
    return int(np.argmax(s)) if best > 0 else 0               # argmax: the first maximum


def _ints(rng, nk, sps, lo, hi):
    return rng.integers(lo, hi + 1, (nk, sps)).astype(np.float64)


def cdr_rows(sps: int, n: int, nch: int = CDR_NCH):
    """x[nch][n] f32, kinds[nch] (names of CDR_KINDS) and want{row: offset} for the rows whose answer
    follows from how they were built. Row r is of kind r % 10; the three non-finite kinds need two
    whole symbols (n >= 2 * sps) and are "gauss" rows otherwise."""
    nk = n // sps
    x = np.zeros((nch, n), np.float32)
    kinds, want = [], {}
    for r in range(nch):
        rng = np.random.default_rng(1000 * sps + 7 * n + r)
        kind = CDR_KINDS[r % len(CDR_KINDS)]
        if kind in ("nan", "inf2", "range") and n < 2 * sps:
            kind = "gauss"
        sign = rng.choice([-1.0, 1.0], (nk, sps))
        tail = 2.6 * rng.standard_normal(n - nk * sps)        # samples past the last whole symbol: unused
        if kind == "gauss":
            row = 2.6 * rng.standard_normal(n)
        elif kind == "zero":
            row, want[r] = np.zeros(n), 0
        elif kind == "subone":
            row, want[r] = rng.uniform(-0.999, 0.999, n), 0
        elif kind == "big":
            row = np.concatenate([(sign * rng.uniform(2.9e6, 3.1e6, (nk, sps))).reshape(-1), tail * 1e6])
        else:
            a = _ints(rng, nk, sps, 0, 3)
            if kind == "tie":                                  # two columns with the same, largest sum
                lo, hi = sorted(int(c) for c in rng.choice(sps, 2, replace=False)) if sps > 1 else (0, 0)
                a[:, lo] = rng.integers(6, 10, nk)
                a[:, hi] = a[:, lo]
                want[r] = lo if nk else 0
            elif kind == "last":
                a[:, sps - 1] = 9
                want[r] = sps - 1 if nk else 0
            elif kind == "first":
                a[:, 0] = 9
                want[r] = 0
            a = a * sign
            if kind in ("nan", "inf2", "range"):
                c0, c1 = (int(c) for c in rng.choice(sps, 2, replace=False)) if sps > 1 else (0, 0)
                a[:, c0] = 9 * sign[:, c0]                     # the otherwise best column
                a[:, c1] = 7 * sign[:, c1] if c1 != c0 else a[:, c1]
                if kind == "nan":
                    a[int(rng.integers(nk)), c0] = np.nan      # + 2^31: the sum turns negative
                elif kind == "inf2":
                    a[0, c0] = a[nk - 1, c0] = np.inf          # + 2^32: the sum wraps to the rest
                else:
                    a[0, c0], a[nk - 1, c1] = 3e9, -3e9
            row = np.concatenate([a.reshape(-1), tail])
        x[r] = row.astype(np.float32)
        kinds.append(kind)
    return x, kinds, want


def cdr_finite(kinds):
    return [k not in ("nan", "inf2", "range") for k in kinds]
