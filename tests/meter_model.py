"""CPU model of the reception meter (include/sdr_amd.h, sdr_meter_*): a numpy f32 restatement of the
readings over the oracle's rows -- Channel.frontend, stereo(..)["pilot"], rds(..)["rds_band"] and
["rds_clean"], orc.cdr, orc.fir_decim, orc.bpf -- with the meter's summation order, and a Python
restatement of sdr_meter_status. Every float is meant to equal the GPU's bit for bit."""
from __future__ import annotations

import math

import numpy as np

ROW_DTYPE = np.dtype([(n, "<f4") for n in ("fm_sum", "fm_sq", "fm_peak", "pilot_sq", "noise_sq", "rds_sq", "eye_abs",
                                           "eye_sq")] +
                     [(n, "<i4") for n in ("eye_n", "flags", "l_peak", "r_peak")] +
                     [(n, "<u8") for n in ("l_sq", "r_sq")])
FLOAT_FIELDS = tuple(n for n in ROW_DTYPE.names if ROW_DTYPE[n] == np.float32)
INT_FIELDS = tuple(n for n in ROW_DTYPE.names if n not in FLOAT_FIELDS)
ROW_AUDIO, ROW_RDS = 1, 2
STEREO, RDS, OFFTUNE, DEAD_AIR = 1, 2, 4, 8
DEFAULTS = dict(pilot_nr_min=1.0, rds_nr_min=4.0, offtune_min=0.25, silence_peak=64)
BLOCK_IF = {0: 7350, 1: 13230, 2: 8000, 3: 12800}
NOISE_TAPS, NOISE_D = 101, 5


def tree_sum(v, parts: int = 256) -> np.float32:
    """The meter's float sum: partial p adds the elements i = p (mod parts) in ascending i from +0
    (all partials at once, a row of `parts` elements per step; the +0 padding of the last row changes
    nothing), then the pairing levels P[p] = fl(P[p] + P[p + w]), w = parts / 2 .. 1."""
    v = np.ascontiguousarray(v, np.float32)
    steps = -(-v.size // parts)
    pad = np.zeros(steps * parts, np.float32)
    pad[:v.size] = v
    P = np.zeros(parts, np.float32)
    for r in pad.reshape(steps, parts):
        P = P + r
    w = parts // 2
    while w >= 1:
        P = P[:w] + P[w:2 * w]
        w //= 2
    assert P.dtype == np.float32
    return P[0]


def sq(v):
    v = np.asarray(v, np.float32)
    return v * v


class ChannelMeter:
    """The model of one channel: block by block, the row the two meter calls write."""

    def __init__(self, orc, mode: int = 0):
        self.orc = orc
        self.ch = orc.Channel(mode, True)
        self.mode = mode
        self.h = orc.bpf(float(self.ch.state.if_Fs), 75e3, 84e3, NOISE_TAPS)
        self.state = np.zeros(NOISE_TAPS - 1, np.float32)     # x[-100..-1]: the previous block's tail

    def audio(self, row, fm, pilot, lr):
        with np.errstate(all="ignore"):
            row["fm_sum"] = tree_sum(fm)
            row["fm_sq"] = tree_sum(sq(fm))
            row["fm_peak"] = np.fmax.reduce(np.abs(fm), initial=np.float32(0))
            row["pilot_sq"] = tree_sum(sq(pilot))
            y = self.orc.fir_decim(fm, self.h, self.state, NOISE_D)   # (keeps the tail for the next block)
            row["noise_sq"] = tree_sum(sq(y))
        if lr is not None:
            for name, s in (("l", lr[0::2].astype(np.int64)), ("r", lr[1::2].astype(np.int64))):
                row[name + "_peak"] = np.abs(s).max()
                row[name + "_sq"] = int((s * s).sum())
        row["flags"] |= ROW_AUDIO

    def rds(self, row, rds_band, rds_clean):
        sps = self.ch.symbol_Fs
        off = self.orc.cdr(sps, rds_clean)
        with np.errstate(all="ignore"):
            row["rds_sq"] = tree_sum(sq(rds_band))
            s = np.abs(rds_clean[off::sps])
            row["eye_abs"] = tree_sum(s, 64)
            row["eye_sq"] = tree_sum(sq(s), 64)
        row["eye_n"] = s.size
        row["flags"] |= ROW_RDS

    def block_fm(self, fm, with_lr: bool = True):
        """One block from its fm_demod row: (row, lr, rds result of the oracle)."""
        row = np.zeros((), ROW_DTYPE)
        lr, d = self.ch.stereo(fm, intermediates=True)
        r = self.ch.rds(fm, intermediates=True)
        self.audio(row, fm, d["pilot"], lr if with_lr else None)
        self.rds(row, r["rds_band"], r["rds_clean"])
        return row, lr, r

    def block(self, iq, with_lr: bool = True):
        return self.block_fm(self.ch.frontend(iq), with_lr)


def run_rows(orc, mode: int, iq_blocks) -> np.ndarray:
    """rows [nblocks] of one channel over iq_blocks [nblocks][2 * block_iq]."""
    m = ChannelMeter(orc, mode)
    return np.stack([m.block(iq)[0] for iq in iq_blocks])


def run_rows_fm(orc, mode: int, fm_blocks) -> np.ndarray:
    m = ChannelMeter(orc, mode)
    return np.stack([m.block_fm(np.ascontiguousarray(fm, np.float32))[0] for fm in fm_blocks])


def _ratio(num: float, den: float) -> float:
    if not (num != 0.0):
        return 0.0
    if den <= 0.0:
        return math.inf if num > 0.0 else 0.0
    return num / den


def _db(x: float) -> float:
    if x > 0.0:
        return 10.0 * math.log10(x)
    return -math.inf if x == 0.0 else math.nan


def status(mode: int, row, **opts) -> dict:
    """sdr_meter_status in Python floats (IEEE double, the same operations in the same order)."""
    o = dict(DEFAULTS, **opts)
    f32 = lambda v: float(np.float32(v))
    n = float(BLOCK_IF[mode])
    n5 = float(BLOCK_IF[mode] // NOISE_D)
    noise = float(row["noise_sq"]) / n5
    out = {"offset": float(row["fm_sum"]) / n, "level_db": _db(float(row["fm_sq"]) / n),
           "pilot_nr": _ratio(float(row["pilot_sq"]) / n, noise), "rds_nr": _ratio(float(row["rds_sq"]) / n, noise)}
    eye = 0.0
    if int(row["eye_n"]) > 0:
        m1 = float(row["eye_abs"]) / int(row["eye_n"])
        m2 = float(row["eye_sq"]) / int(row["eye_n"])
        eye = _ratio(m1 * m1, m2 - m1 * m1)
    out["eye_db"] = _db(eye)
    f = 0
    if out["pilot_nr"] >= f32(o["pilot_nr_min"]):
        f |= STEREO
    if out["rds_nr"] >= f32(o["rds_nr_min"]):
        f |= RDS
    if abs(out["offset"]) >= f32(o["offtune_min"]):
        f |= OFFTUNE
    if (int(row["flags"]) & ROW_AUDIO) and int(row["l_peak"]) <= o["silence_peak"] and int(row["r_peak"]) <= o["silence_peak"]:
        f |= DEAD_AIR
    out["flags"] = f
    return out


def same_rows(got, want) -> list:
    """The fields in which two row arrays differ, floats compared as uint32: [] when equal."""
    got, want = np.asarray(got), np.asarray(want)
    bad = []
    for name in FLOAT_FIELDS:
        if not np.array_equal(np.ascontiguousarray(got[name]).view(np.uint32),
                              np.ascontiguousarray(want[name]).view(np.uint32)):
            bad.append(name)
    for name in INT_FIELDS:
        if not np.array_equal(got[name], want[name]):
            bad.append(name)
    return bad
