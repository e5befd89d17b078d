"""CPU model of the wideband splitter (include/sdr_amd.h, sdr_split_*), shared by the splitter tests.
Not a conftest.

The definition is all integer. The model forms, per output sample, the window of 2 T input bytes and
multiplies it by the [2 T x 2 R] tap matrix in float64 BLAS: every product is below 2^21 and every sum
below 2^28 in magnitude, far under 2^53, so the float64 GEMM is exact whatever its summation order. The
sign flip, the rounding shift, the clamp and the clip counters are int64 numpy. The tap table is
computed here from the formula, independently of the library's."""
from __future__ import annotations

import numpy as np

GEOM = {0: (2400, 73500), 1: (1440, 52920), 2: (2400, 80000), 3: (1152, 38400)}   # mode: (N, block_iq)
SHIFT_DEFAULT = {4: 14, 8: 15, 10: 16}


def taps_f64(W: int):
    """(re, im) float64 [R][T] before rounding: 8191 h cos(theta), 8191 h sin(theta)."""
    T, R = 16 * W, 2 * W - 1
    m = np.arange(T, dtype=np.int64)
    u = m.astype(np.float64) - (T - 1) / 2.0
    x = u / W
    sinc = np.sin(np.pi * x) / (np.pi * x)
    win = 0.42 - 0.5 * np.cos(2.0 * np.pi * (m + 0.5) / T) + 0.08 * np.cos(4.0 * np.pi * (m + 0.5) / T)
    h = sinc * win
    k = (np.arange(R, dtype=np.int64) - (W - 1))[:, None]
    a = np.mod(k * (2 * m - T + 1)[None, :], 4 * W)               # reduced first, to [0, 4 W)
    th = np.pi * a.astype(np.float64) / (2 * W)
    return 8191.0 * h[None, :] * np.cos(th), 8191.0 * h[None, :] * np.sin(th)


def taps(W: int) -> np.ndarray:
    """int16 [R][T][2] (g_re, g_im)."""
    re, im = taps_f64(W)
    return np.stack([np.rint(re), np.rint(im)], axis=-1).astype(np.int16)


def tap_matrix(W: int) -> np.ndarray:
    """float64 [2 T][2 R]: row 2 s + c is byte c (I, Q) of the window's sample s (sample W t - T + 1 + s,
    tap m = T - 1 - s), column 2 r + p is acc_re (p = 0) or acc_im (p = 1) of row r."""
    g = taps(W).astype(np.float64)
    T, R = 16 * W, 2 * W - 1
    M = np.zeros((2 * T, 2 * R))
    gre, gim = g[:, ::-1, 0].T, g[:, ::-1, 1].T                   # [s][r], m = T - 1 - s
    M[0::2, 0::2] = gre
    M[1::2, 0::2] = -gim
    M[0::2, 1::2] = gim
    M[1::2, 1::2] = gre
    return M


class SplitModel:
    """One stream's splitter: block(wide int8 [2 W block_iq]) -> (rows u8 [R][2 block_iq]); clips int64 [R]."""

    CHUNK = 8192

    def __init__(self, mode: int, W: int, shift=None):
        assert W in (4, 8, 10)
        self.N, self.block_iq = GEOM[mode]
        self.W, self.T, self.R = W, 16 * W, 2 * W - 1
        self.shift = SHIFT_DEFAULT[W] if shift is None else int(shift)
        self.M = tap_matrix(W)
        self.k = np.arange(self.R, dtype=np.int64) - (W - 1)
        self.reset()

    def reset(self):
        self.hist = np.zeros(2 * (self.T - 1), np.int8)
        self.clips = np.zeros(self.R, np.int64)
        self.t0 = 0

    def acc(self, wide: np.ndarray) -> np.ndarray:
        """int64 [block_iq][2 R] of one block, before the sign flip; advances the history."""
        W, T, b = self.W, self.T, self.block_iq
        assert wide.shape == (2 * W * b,) and wide.dtype == np.int8
        x = np.concatenate([self.hist, wide])                      # byte 0 is sample -(T - 1) of the block
        out = np.empty((b, 2 * self.R), np.int64)
        for c0 in range(0, b, self.CHUNK):
            n = min(self.CHUNK, b - c0)
            win = np.lib.stride_tricks.as_strided(x[2 * W * c0:], shape=(n, 2 * T), strides=(2 * W, 1))
            y = win.astype(np.float64) @ self.M
            out[c0:c0 + n] = y.astype(np.int64)
            assert np.array_equal(out[c0:c0 + n].astype(np.float64), y)
        self.hist = x[-2 * (T - 1):].copy()
        return out

    def flipped(self, wide: np.ndarray) -> np.ndarray:
        """int64 [block_iq][2 R] of one block with the sign flip on odd k t applied; advances t."""
        b = self.block_iq
        acc = self.acc(np.ascontiguousarray(wide))
        t = self.t0 + np.arange(b, dtype=np.int64)
        odd = ((self.k[None, :] * t[:, None]) & 1) == 1            # [b][R]
        self.t0 += b
        return np.where(np.repeat(odd, 2, axis=1), -acc, acc)

    def block(self, wide: np.ndarray) -> np.ndarray:
        rows, over = finish(self.flipped(wide), self.shift)
        self.clips += over
        return rows


def finish(acc: np.ndarray, shift: int):
    """(rows u8 [R][2 b], clips int64 [R]) of the flipped sums int64 [b][2 R] of one block."""
    b, R = acc.shape[0], acc.shape[1] // 2
    v = 128 + ((acc + (1 << (shift - 1))) >> shift)                # numpy's >> on int64 is arithmetic
    over = ((v < 0) | (v > 255)).reshape(b, R, 2).sum(axis=(0, 2))
    rows = np.ascontiguousarray(np.clip(v, 0, 255).astype(np.uint8).reshape(b, R, 2).transpose(1, 0, 2))
    return rows.reshape(R, 2 * b), over


def sums(mode: int, W: int, wide: np.ndarray) -> np.ndarray:
    """wide int8 [nblocks][nwide][2 W block_iq] -> the flipped sums int64 [nblocks][nwide][block_iq][2 R]
    (what every shift starts from)."""
    nblocks, nwide = wide.shape[0], wide.shape[1]
    ms = [SplitModel(mode, W) for _ in range(nwide)]
    return np.stack([np.stack([ms[w].flipped(wide[b, w]) for w in range(nwide)]) for b in range(nblocks)])


def finish_all(acc: np.ndarray, shift: int):
    """sums() -> (rows u8 [nblocks][nwide R][2 block_iq], clips int64 [nwide][R])."""
    nblocks, nwide = acc.shape[0], acc.shape[1]
    clips = np.zeros((nwide, acc.shape[3] // 2), np.int64)
    rows = []
    for b in range(nblocks):
        rb = []
        for w in range(nwide):
            r, o = finish(acc[b, w], shift)
            rb.append(r)
            clips[w] += o
        rows.append(np.concatenate(rb))
    return np.stack(rows), clips


def run(mode: int, W: int, wide: np.ndarray, shift=None):
    """wide int8 [nblocks][nwide][2 W block_iq] -> (rows u8 [nblocks][nwide R][2 block_iq], clips [nwide][R])."""
    return finish_all(sums(mode, W, wide), SHIFT_DEFAULT[W] if shift is None else int(shift))


# ------------------------------------------------------------------ the wide picker
def wide_pick(mode: int, W: int, psd_rows, pick, first_khz: int = 0, step_khz: int = 100, **opts):
    """The wide scan's rule over the psd rows [nwide R][N] of a batch: each row is picked with
    guard_khz = N / 4 (candidates |khz| <= N / 4) on the absolute station grid, first_khz of row k being
    (first - k N / 2) mod step, and a pick whose absolute frequency an earlier row of the same stream
    already gave (the |khz| = N / 4 tie) is dropped. `pick` is scan_model.pick or a wrapper of
    pkg.scan_pick with its signature. Returns [(src, khz)] with src = w R + r, row after row."""
    N = GEOM[mode][0]
    R = 2 * W - 1
    out = []
    for w in range(len(psd_rows) // R):
        seen = set()
        for r in range(R):
            k = r - (W - 1)
            centre = k * N // 2
            khz, _ = pick(psd_rows[w * R + r], guard_khz=N // 4, step_khz=step_khz,
                          first_khz=(first_khz - centre) % step_khz, **opts)
            for f in khz:
                if centre + int(f) not in seen:
                    seen.add(centre + int(f))
                    out.append((w * R + r, int(f)))
    return out


# ------------------------------------------------------------------ the composite wide capture
_WIDE: dict = {}


def wide_composite(synth_mod, W: int, nblocks: int, offsets_khz, mode: int = 0):
    """(int8 [nblocks][2 W block_iq], clipped count): three FMMultiplexSource(c, fs = W * 2.4e6) stations,
    each taken to floats as (u8 - 128) / 127, scaled by 1/3, shifted to offsets_khz of the wide capture's
    centre by an integer-indexed rotator of W * 2400 entries, summed and quantised round(127 z) to int8."""
    key = (W, nblocks, tuple(offsets_khz), mode)
    if key not in _WIDE:
        assert mode == 0 and len(offsets_khz) == 3
        NW = W * 2400
        blk = W * GEOM[mode][1]
        ang = 2.0 * np.pi * np.arange(NW, dtype=np.float64) / NW
        rot = np.cos(ang) + 1j * np.sin(ang)
        n = np.arange(nblocks * blk, dtype=np.int64)
        z = np.zeros(nblocks * blk, np.complex128)
        for c, f in enumerate(offsets_khz):
            src = synth_mod.FMMultiplexSource(c, fs=W * 2400000)
            u = np.concatenate([src.next_block(blk) for _ in range(nblocks)]).astype(np.float64)
            x = ((u[0::2] - 128.0) + 1j * (u[1::2] - 128.0)) / 127.0
            z += (x / 3.0) * rot[np.mod(np.int64(f) * n, NW)]
        q = np.empty(2 * z.size, np.float64)
        q[0::2] = np.round(127.0 * z.real)
        q[1::2] = np.round(127.0 * z.imag)
        clipped = int(np.count_nonzero((q < -128) | (q > 127)))
        _WIDE[key] = (np.clip(q, -128, 127).astype(np.int8).reshape(nblocks, 2 * blk), clipped)
    return _WIDE[key]
