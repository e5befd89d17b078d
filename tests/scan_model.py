"""CPU model of the band scan (include/sdr_amd.h, sdr_scan_*), shared by the scan tests. Not a conftest.

The spectrum is float64: x = (u8 - 128) / 128 exact, w the f32 Hann table of pkg.scan_window cast to
f64, per segment np.fft.fft(x * w) (numpy's forward transform is e^(-j 2 pi k n / N), the scan's
sign) and |X|^2. The picker is a plain restatement of the rule in the header."""
from __future__ import annotations

import numpy as np

from tuner_model import composite  # noqa: F401  (the composite capture, for the scan tests)

U = 2.0 ** -24          # f32 unit round-off
E_REL = 2.0 ** -16      # per-segment DFT error bound relative to ||xw||_1 (tests/test_gpu_scan.py)


def segments(pkg, mode: int, row: np.ndarray) -> np.ndarray:
    """xw [S_b][N] complex128 of one block's u8 row [2*block_iq]."""
    N, S, block_iq = pkg.scan_geometry(mode)
    assert row.shape == (2 * block_iq,) and row.dtype == np.uint8
    x = (row.astype(np.float64) - 128.0) / 128.0
    z = (x[0::2] + 1j * x[1::2])[:S * N].reshape(S, N)
    return z * pkg.scan_window(mode).astype(np.float64)[None, :]


def block_power(pkg, mode: int, row: np.ndarray):
    """(A_ref [N], tol [N]) of one block of one row: A_ref = sum_s |X_s|^2 and the first part of the
    tolerance, sum_s (2 |X_s| e_s + e_s^2) with e_s = 2^-16 ||xw_s||_1. The accumulation term
    (S + 6) 2^-24 A_ref is added by the caller, who knows the total S."""
    xw = segments(pkg, mode, row)
    X = np.fft.fft(xw, axis=1)
    e = E_REL * np.abs(xw).sum(axis=1)                                # 2^-16 sum_n |xw_n|
    A = (X.real ** 2 + X.imag ** 2).sum(axis=0)
    tol = (2.0 * np.abs(X) * e[:, None] + (e ** 2)[:, None]).sum(axis=0)
    return A, tol


def rows_power(pkg, mode: int, blocks):
    """The model over several blocks of a batch: blocks = list of [nrows][2*block_iq] u8 arrays.
    Returns (A_ref [nrows][N], tol [nrows][N], S) with the accumulation term included."""
    N, S_b, _ = pkg.scan_geometry(mode)
    nrows = blocks[0].shape[0]
    A = np.zeros((nrows, N))
    tol = np.zeros((nrows, N))
    for blk in blocks:
        for r in range(nrows):
            a, t = block_power(pkg, mode, np.ascontiguousarray(blk[r, :2 * pkg.scan_geometry(mode)[2]]))
            A[r] += a
            tol[r] += t
    S = S_b * len(blocks)
    return A, tol + (S + 6) * U * A, S


DEFAULTS = dict(half_width_khz=100, step_khz=100, first_khz=0, sep_khz=150, guard_khz=100, thr_db=10.0)


def pick(psd_row, **opts):
    """The picker rule restated: (khz list, db list) in descending C, ties in ascending khz."""
    o = dict(DEFAULTS)
    o.update(opts)
    p = np.asarray(psd_row, np.float32).astype(np.float64)
    N = p.size
    W, step, first, sep, guard = (o[k] for k in ("half_width_khz", "step_khz", "first_khz", "sep_khz", "guard_khz"))
    thr = float(np.float32(o["thr_db"]))
    C = np.zeros(N)
    for d in range(-W, W + 1):                       # ascending d, like the library
        C = C + np.roll(p, -d)                       # np.roll(p, -d)[k] = p[(k + d) mod N]
    F = np.sort(C)[(N - 1) // 2]
    need = F * 10.0 ** (thr / 10.0)
    cand = [f for f in range(-N // 2 + guard, N // 2 - guard + 1) if (f - first) % step == 0]
    found = []
    for f in cand:
        c = C[f % N]
        if not (c > 0 and c >= need):
            continue
        beaten = any(g != f and abs(g - f) <= sep and (C[g % N] > c or (C[g % N] == c and g < f)) for g in cand)
        if not beaten:
            found.append((f, c))
    found.sort(key=lambda fc: (-fc[1], fc[0]))
    with np.errstate(divide="ignore"):
        db = [float(np.float32(10.0 * np.log10(c / F))) if F > 0 else float("inf") for _, c in found]
    return [f for f, _ in found], db
