"""CPU model of the 16-bit wideband splitter (include/sdr_amd.h, sdr_split16_*), shared by its tests.
Not a conftest.

Built on split_model: its tap table and tap matrix are the definition's, imported, not copied. The sums are
formed as there, by a float64 GEMM of each output's window with the tap matrix; with 16-bit samples every
product is below 2^28 and every sum below 2^33 in magnitude (asserted per W in bounds()), far under 2^53, so
the GEMM is exact whatever its summation order, and every block asserts that it was. The sign flip, the shift
per row, the clamp, the clip counters, the peaks and the gain rule are int64 numpy or plain Python integers."""
from __future__ import annotations

import numpy as np

from split_model import GEOM, SHIFT_DEFAULT as SHIFT_DEFAULT_S8, tap_matrix, taps   # noqa: F401 (taps: re-exported)

SHIFT_DEFAULT = {W: s + 8 for W, s in SHIFT_DEFAULT_S8.items()}    # 22, 23, 24: the same gain relative to full scale
SHIFT_MAX = 33
TARGET_DEFAULT = 90
COL_ABS_MAX = {4: 75012, 8: 148820, 10: 185844}                     # max over columns of sum |e| (include/sdr_amd.h)


def bounds(W: int):
    """(max_col sum |e|, the largest |acc| any int16 capture can give): asserted against the header's figures,
    under 2^33 and over 2^31."""
    col = int(np.abs(tap_matrix(W)).sum(axis=0).max())
    assert col == COL_ABS_MAX[W]
    top = 32768 * col
    assert 2 ** 31 < top < 2 ** 33
    return col, top


class Split16Model:
    """One stream's splitter: flipped(wide int16 [2 W block_iq]) -> int64 [block_iq][2 R]."""

    CHUNK = 8192

    def __init__(self, mode: int, W: int):
        assert W in (4, 8, 10)
        self.N, self.block_iq = GEOM[mode]
        self.W, self.T, self.R = W, 16 * W, 2 * W - 1
        self.M = tap_matrix(W)
        self.k = np.arange(self.R, dtype=np.int64) - (W - 1)
        self.top = bounds(W)[1]
        self.reset()

    def reset(self):
        self.hist = np.zeros(2 * (self.T - 1), np.int16)
        self.t0 = 0

    def acc(self, wide: np.ndarray, n_out=None) -> np.ndarray:
        """int64 [n_out][2 R] of a piece of W n_out samples, before the sign flip; advances the history. (The
        splitter's own pieces are blocks of block_iq outputs; any other cut gives the same sums.)"""
        W, T = self.W, self.T
        b = self.block_iq if n_out is None else n_out
        assert wide.shape == (2 * W * b,) and wide.dtype == np.int16
        x = np.concatenate([self.hist, wide])                      # value 0 is sample -(T - 1) of the piece
        out = np.empty((b, 2 * self.R), np.int64)
        for c0 in range(0, b, self.CHUNK):
            n = min(self.CHUNK, b - c0)
            win = np.lib.stride_tricks.as_strided(x[2 * W * c0:], shape=(n, 2 * T), strides=(2 * W * 2, 2))
            y = win.astype(np.float64) @ self.M
            out[c0:c0 + n] = y.astype(np.int64)
            assert np.array_equal(out[c0:c0 + n].astype(np.float64), y) and np.abs(y).max() <= self.top
        self.hist = x[-2 * (T - 1):].copy()
        return out

    def flipped(self, wide: np.ndarray, n_out=None) -> np.ndarray:
        """int64 [n_out][2 R] with the sign flip on odd k t applied; advances t."""
        acc = self.acc(np.ascontiguousarray(wide), n_out)
        b = acc.shape[0]
        t = self.t0 + np.arange(b, dtype=np.int64)
        odd = ((self.k[None, :] * t[:, None]) & 1) == 1            # [b][R]
        self.t0 += b
        return np.where(np.repeat(odd, 2, axis=1), -acc, acc)


def finish(acc: np.ndarray, shifts):
    """(rows u8 [R][2 b], clips int64 [R], peaks int64 [R]) of the flipped sums int64 [b][2 R] of one block;
    shifts: one int or [R]."""
    b, R = acc.shape[0], acc.shape[1] // 2
    s = np.broadcast_to(np.asarray(shifts, np.int64), (R,))
    assert s.min() >= 1 and s.max() <= SHIFT_MAX
    s2 = np.repeat(s, 2)[None, :]
    v = 128 + ((acc + (np.int64(1) << (s2 - 1))) >> s2)             # numpy's >> on int64 is arithmetic
    over = ((v < 0) | (v > 255)).reshape(b, R, 2).sum(axis=(0, 2))
    peaks = np.abs(acc).reshape(b, R, 2).max(axis=(0, 2))
    rows = np.ascontiguousarray(np.clip(v, 0, 255).astype(np.uint8).reshape(b, R, 2).transpose(1, 0, 2))
    return rows.reshape(R, 2 * b), over, peaks


def sums(mode: int, W: int, wide: np.ndarray) -> np.ndarray:
    """wide int16 [nblocks][nwide][2 W block_iq] -> the flipped sums int64 [nblocks][nwide][block_iq][2 R]
    (what every shift table starts from)."""
    nblocks, nwide = wide.shape[0], wide.shape[1]
    ms = [Split16Model(mode, W) for _ in range(nwide)]
    return np.stack([np.stack([ms[w].flipped(wide[b, w]) for w in range(nwide)]) for b in range(nblocks)])


def finish_all(acc: np.ndarray, shifts):
    """sums() -> (rows u8 [nblocks][nwide R][2 block_iq], clips int64 [nwide][R], peaks int64 [nwide][R]);
    shifts: one int, [nwide][R], or [nblocks][nwide][R] (a table per block)."""
    nblocks, nwide, R = acc.shape[0], acc.shape[1], acc.shape[3] // 2
    tab = np.broadcast_to(np.asarray(shifts, np.int64), (nblocks, nwide, R))
    clips = np.zeros((nwide, R), np.int64)
    peaks = np.zeros((nwide, R), np.int64)
    rows = []
    for b in range(nblocks):
        rb = []
        for w in range(nwide):
            r, o, p = finish(acc[b, w], tab[b, w])
            rb.append(r)
            clips[w] += o
            peaks[w] = np.maximum(peaks[w], p)
        rows.append(np.concatenate(rb))
    return np.stack(rows), clips, peaks


def run(mode: int, W: int, wide: np.ndarray, shifts=None):
    return finish_all(sums(mode, W, wide), SHIFT_DEFAULT[W] if shifts is None else shifts)


# ------------------------------------------------------------------ the gain rule
def rnd(p: int, s: int) -> int:
    return (int(p) + (1 << (s - 1))) >> s


def shift_for(peak: int, target: int = TARGET_DEFAULT, W: int = 8) -> int:
    """The smallest s in 1..33 with rnd(peak, s) <= target; W's default for peak == 0."""
    assert 1 <= target <= 127 and peak >= 0
    if peak == 0:
        return SHIFT_DEFAULT[W]
    for s in range(1, SHIFT_MAX):
        if rnd(peak, s) <= target:
            return s
    return SHIFT_MAX


def shifts_for(peaks: np.ndarray, target: int = TARGET_DEFAULT, W: int = 8) -> np.ndarray:
    return np.array([shift_for(int(p), target, W) for p in peaks.ravel()], np.int64).reshape(peaks.shape)


# ------------------------------------------------------------------ widening an s8 capture
def widen256(wide8: np.ndarray) -> np.ndarray:
    return (wide8.astype(np.int16) * 256).astype(np.int16)


def sign_extend(wide8: np.ndarray) -> np.ndarray:
    return wide8.astype(np.int16)


# ------------------------------------------------------------------ the composite wide capture
_WIDE: dict = {}


def wide_composite16(synth_mod, W: int, nblocks: int, offsets_khz, amps, mode: int = 0, tone=None):
    """(int16 [nblocks][2 W block_iq], int8 the same, clipped count of either): FMMultiplexSource(c, fs = W * 2.4e6)
    stations as split_model.wide_composite makes them, station c scaled by amps[c], summed; the same sum z
    quantised round(32767 z) to int16 and round(127 z) to int8. tone = (khz, amp) adds a station made in float64
    here, amp exp(j (75 sin(2 pi 1 kHz t))) at khz: a 1 kHz tone at 75 kHz deviation with no noise and no 8-bit
    steps of its own (an FMMultiplexSource station carries both, at a level an s8 capture's own steps do not
    exceed by much: next to it the two captures would differ little)."""
    key = (W, nblocks, tuple(offsets_khz), tuple(amps), mode, tone)
    if key not in _WIDE:
        assert mode == 0 and len(offsets_khz) == len(amps)
        NW = W * 2400
        blk = W * GEOM[mode][1]
        ang = 2.0 * np.pi * np.arange(NW, dtype=np.float64) / NW
        rot = np.cos(ang) + 1j * np.sin(ang)
        n = np.arange(nblocks * blk, dtype=np.int64)
        z = np.zeros(nblocks * blk, np.complex128)
        for c, (f, a) in enumerate(zip(offsets_khz, amps)):
            src = synth_mod.FMMultiplexSource(c, fs=W * 2400000)
            u = np.concatenate([src.next_block(blk) for _ in range(nblocks)]).astype(np.float64)
            x = ((u[0::2] - 128.0) + 1j * (u[1::2] - 128.0)) / 127.0
            z += (x * a) * rot[np.mod(np.int64(f) * n, NW)]
        if tone is not None:
            z += tone[1] * np.exp(1j * 75.0 * np.sin(ang[np.mod(n, NW)])) * rot[np.mod(np.int64(tone[0]) * n, NW)]
        out, clipped = [], 0
        for full, lo, hi, dt in ((32767.0, -32768, 32767, np.int16), (127.0, -128, 127, np.int8)):
            q = np.empty(2 * z.size, np.float64)
            q[0::2] = np.round(full * z.real)
            q[1::2] = np.round(full * z.imag)
            clipped += int(np.count_nonzero((q < lo) | (q > hi)))
            out.append(np.clip(q, lo, hi).astype(dt).reshape(nblocks, 2 * blk))
        _WIDE[key] = (out[0], out[1], clipped)
    return _WIDE[key]
