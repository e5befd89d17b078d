"""CPU model of the shared-capture tuner (include/sdr_amd.h, sdr_tuner_set / sdr_frontend_tuned),
shared by the tuner tests. Not a conftest.

The mixer is numpy float32 arithmetic, whose *, + and - round separately (four products, two sums,
no FMA), with the rotator index in int64 and the table from pkg.tuner_table; the FIR, discriminator
and every later stage are the oracle's (oracle.fir_decim with oracle.lpf(rf_Fs, 1e5, 101) and
100-sample states, oracle.fm_demod, oracle.Channel(mode).mono / stereo / rds)."""
from __future__ import annotations

import numpy as np

from conftest import channel_input

NTAPS = 101
# the composite capture: FMMultiplexSource(c), c = 0, 1, 2, at these offsets from the capture's centre
COMPOSITE_KHZ = (-600, 0, 500)
COMPOSITE_BLOCKS = 10


class TunedRow:
    """The per-source-row state: the row's last 100 u8 pairs (u8 128 before the first block)."""

    def __init__(self):
        self.tail = np.full(2 * (NTAPS - 1), 128, np.uint8)


class TunedChannel:
    """One tuned channel: mixer + FIR + discriminator block by block, then the oracle's stages."""

    def __init__(self, pkg, oracle, mode: int, khz: int, rds_on: bool = True):
        self.oracle = oracle
        self.chan = oracle.Channel(mode, rds_on)
        st = self.chan.state
        self.rf_Fs, self.D = st.rf_Fs, st.rf_decim
        self.block_iq = self.chan.block_iq
        self.N = self.rf_Fs // 1000
        self.table = pkg.tuner_table(mode)
        assert self.table.shape == (self.N, 2)
        self.h = oracle.lpf(float(self.rf_Fs), 1e5, NTAPS)
        self.khz = int(khz)
        self.prev = np.zeros(2, np.float32)
        self.block = 0

    def _mix(self, u8pairs: np.ndarray, n0: int):
        """(y_I, y_Q) of interleaved u8 I/Q whose first sample is sample n0 of the stream."""
        x = (u8pairs.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
        xi, xq = x[0::2], x[1::2]
        n = np.int64(n0) + np.arange(xi.size, dtype=np.int64)
        i = np.mod(np.int64(self.khz) * n, np.int64(self.N))       # mathematical, non-negative
        c, s = self.table[i, 0], self.table[i, 1]
        yi = xi * c + xq * s
        yq = xq * c - xi * s
        assert yi.dtype == np.float32 and yq.dtype == np.float32
        return yi, yq

    def frontend(self, row: TunedRow, iq: np.ndarray) -> np.ndarray:
        """fm_demod of this block; the caller updates row.tail after every channel of the row ran."""
        n0 = self.block * self.block_iq
        hi, hq = self._mix(row.tail, n0 - (NTAPS - 1))
        yi, yq = self._mix(iq, n0)
        # oracle.fir_decim's state is the previous block's last samples in order; it updates its copy
        I = self.oracle.fir_decim(yi, self.h, np.ascontiguousarray(hi), self.D)
        Q = self.oracle.fir_decim(yq, self.h, np.ascontiguousarray(hq), self.D)
        fm = self.oracle.fm_demod(I, Q, self.prev)
        self.block += 1
        return fm


def run_tuned(pkg, oracle, mode: int, rows: np.ndarray, src, khz, stages: bool = False, rds_on: bool = True):
    """rows: u8 [nblocks][nsrc][2*block_iq]. Returns per channel a dict of per-block lists: fm and,
    with stages, mono, stereo, rds_clean, bits (None where the block decodes nothing)."""
    nblocks, nsrc = rows.shape[0], rows.shape[1]
    chans = [TunedChannel(pkg, oracle, mode, k, rds_on) for k in khz]
    srows = [TunedRow() for _ in range(nsrc)]
    out = [{"fm": [], "mono": [], "stereo": [], "rds_clean": [], "bits": []} for _ in chans]
    for b in range(nblocks):
        for c, ch in enumerate(chans):
            fm = ch.frontend(srows[src[c]], rows[b, src[c]])
            out[c]["fm"].append(fm)
            if stages:
                out[c]["mono"].append(ch.chan.mono(fm))
                out[c]["stereo"].append(ch.chan.stereo(fm))
                r = ch.chan.rds(fm)
                out[c]["rds_clean"].append(r["rds_clean"])
                out[c]["bits"].append(r["bits"])
        for r in range(nsrc):
            srows[r].tail = rows[b, r, -2 * (NTAPS - 1):].copy()
    return out


_COMPOSITE: dict = {}


def composite(synth_mod, nblocks: int = COMPOSITE_BLOCKS):
    """(u8 [nblocks][2*block_iq], clipped samples): stations FMMultiplexSource(0..2) taken back to
    floats as (u8 - 128) / 127, scaled by 1/3, shifted up by COMPOSITE_KHZ, summed and requantised
    with round(127 z + 128). Mode 0 (2.4 MS/s: a 1 kHz step is 1/2400 of a turn per sample)."""
    if nblocks not in _COMPOSITE:
        N = 2400
        ang = 2.0 * np.pi * np.arange(N, dtype=np.float64) / N
        rot = np.cos(ang) + 1j * np.sin(ang)
        blk = synth_mod.BLOCK_IQ
        z = np.zeros(nblocks * blk, np.complex128)
        n = np.arange(nblocks * blk, dtype=np.int64)
        for c, k in enumerate(COMPOSITE_KHZ):
            u = channel_input(synth_mod, c, nblocks).reshape(-1).astype(np.float64)
            x = ((u[0::2] - 128.0) + 1j * (u[1::2] - 128.0)) / 127.0
            z += (x / 3.0) * rot[np.mod(np.int64(k) * n, N)]
        q = np.empty(2 * z.size, np.float64)
        q[0::2] = np.round(127.0 * z.real + 128.0)
        q[1::2] = np.round(127.0 * z.imag + 128.0)
        clipped = int(np.count_nonzero((q < 0) | (q > 255)))
        _COMPOSITE[nblocks] = (np.clip(q, 0, 255).astype(np.uint8).reshape(nblocks, 2 * blk), clipped)
    return _COMPOSITE[nblocks]


_MODEL: dict = {}


def composite_model(pkg, oracle, synth_mod, extra=()):
    """The model's outputs for the composite's three stations (+ extra (src, khz) channels on row 0),
    computed once and shared: the tests leave it unchanged."""
    key = tuple(extra)
    if key not in _MODEL:
        rows = composite(synth_mod)[0][:, None, :]
        khz = list(COMPOSITE_KHZ) + [k for _, k in extra]
        _MODEL[key] = run_tuned(pkg, oracle, 0, rows, [0] * len(khz), khz, stages=True)
    return _MODEL[key]
