"""CPU model of the reception meter's RF readings (include/sdr_amd.h, SDR_FLAG_IF_ENVELOPE / sdr_meter_rf /
sdr_meter_rf_status), shared by the RF meter tests. Not a conftest, not a test.

The IF envelope row comes from the oracle's own pieces: oracle.fir_decim with oracle.lpf(rf_Fs, 1e5, 101) on
(u8 - 128) / 128 and 100-sample states (untuned), or the tuner model's mixer in front of the same FIR (tuned);
e = I * I + Q * Q in numpy float32, whose * and + round separately. The rows use meter_model.tree_sum, the
status arithmetic is Python doubles in the order of sdr_meter_rf_status. Every float is meant to equal the GPU's
bit for bit."""
from __future__ import annotations

import math

import numpy as np

import demod_model as dm
import meter_model as mm
import tuner_model as tm

ROW_DTYPE = np.dtype([(n, "<f4") for n in ("env_sum", "env_sq", "env_min", "env_max")] +
                     [("n", "<i4"), ("flags", "<i4"), ("reserved", "<i4", (2,))])
assert ROW_DTYPE.itemsize == 32
FLOAT_FIELDS = ("env_sum", "env_sq", "env_min", "env_max")
ROW_RF = 4
WEAK = 1
RIPPLE_MAX = float(np.float32(21.0) / np.float32(121.0))     # 21.0f / 121.0f
NTAPS = 101
RF_FS = {0: 2400000, 1: 1440000, 2: 2400000, 3: 1152000}
RF_DECIM = {0: 10, 1: 4, 2: 10, 3: 3}


def env(I, Q) -> np.ndarray:
    """fl(fl(I I) + fl(Q Q)) per sample."""
    I, Q = np.asarray(I, np.float32), np.asarray(Q, np.float32)
    e = I * I + Q * Q
    assert e.dtype == np.float32
    return e


class EnvChannel:
    """One untuned channel: the front end's two FIRs block by block, their outputs kept."""

    def __init__(self, orc, mode: int = 0):
        self.orc = orc
        self.D = RF_DECIM[mode]
        self.h = orc.lpf(float(RF_FS[mode]), 1e5, NTAPS)
        self.state_i = np.zeros(NTAPS - 1, np.float32)
        self.state_q = np.zeros(NTAPS - 1, np.float32)

    def iq(self, u8pairs):
        x = (np.asarray(u8pairs).astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
        I = self.orc.fir_decim(np.ascontiguousarray(x[0::2]), self.h, self.state_i, self.D)   # (the states move on)
        Q = self.orc.fir_decim(np.ascontiguousarray(x[1::2]), self.h, self.state_q, self.D)
        return I, Q

    def block(self, u8pairs) -> np.ndarray:
        return env(*self.iq(u8pairs))


class TunedEnvChannel(tm.TunedChannel):
    """The tuner model's channel, keeping I and Q: frontend() returns fm and leaves the block's row in .env.
    phase: the phase discriminator's fm (SDR_FLAG_PHASE_DEMOD) instead of the reference's."""

    def __init__(self, pkg, oracle, mode: int, khz: int, phase: bool = False):
        super().__init__(pkg, oracle, mode, khz)
        self.phase = phase
        self.env = None

    def frontend(self, row, iq):
        n0 = self.block * self.block_iq
        hi, hq = self._mix(row.tail, n0 - (tm.NTAPS - 1))
        yi, yq = self._mix(iq, n0)
        I = self.oracle.fir_decim(yi, self.h, np.ascontiguousarray(hi), self.D)
        Q = self.oracle.fir_decim(yq, self.h, np.ascontiguousarray(hq), self.D)
        self.env = env(I, Q)
        if self.phase:
            fm, self.prev = dm.demod(I, Q, self.prev)
        else:
            fm = self.oracle.fm_demod(I, Q, self.prev)
        self.block += 1
        return fm


def run_tuned_env(pkg, oracle, mode: int, rows, src, khz, phase: bool = False):
    """(fm, env), each [nch][nblocks][block_if], of the model over rows u8 [nblocks][nsrc][2*block_iq]."""
    chans = [TunedEnvChannel(pkg, oracle, mode, k, phase) for k in khz]
    srows = [tm.TunedRow() for _ in range(rows.shape[1])]
    fm, ev = [[] for _ in chans], [[] for _ in chans]
    for b in range(rows.shape[0]):
        for c, ch in enumerate(chans):
            fm[c].append(ch.frontend(srows[src[c]], rows[b, src[c]]))
            ev[c].append(ch.env)
        for r, sr in enumerate(srows):
            sr.tail = rows[b, r, -2 * (tm.NTAPS - 1):].copy()
    return np.asarray(fm), np.asarray(ev)


def rf_row(e) -> np.ndarray:
    """The row sdr_meter_rf writes for the envelope row e."""
    e = np.ascontiguousarray(e, np.float32)
    row = np.zeros((), ROW_DTYPE)
    with np.errstate(all="ignore"):
        row["env_sum"] = mm.tree_sum(e)
        row["env_sq"] = mm.tree_sum(mm.sq(e))
        row["env_max"] = np.fmax.reduce(e, initial=np.float32(0))
        row["env_min"] = np.fmin.reduce(e, initial=np.float32(np.inf))
    row["n"] = e.size
    row["flags"] = ROW_RF
    return row


def run_long(rows) -> np.ndarray:
    """The run-long row of one channel's block rows: env_sum, env_sq and n added in double in block order, the
    minimum of the minima and the maximum of the maxima, the flags ORed; the sums stored as f32 again."""
    rows = np.asarray(rows, ROW_DTYPE).reshape(-1)
    out = np.zeros((), ROW_DTYPE)
    s = q = 0.0
    n = f = 0
    mn, mx = math.inf, 0.0
    for r in rows:
        if not int(r["flags"]) & ROW_RF:
            continue
        s += float(r["env_sum"])
        q += float(r["env_sq"])
        n += int(r["n"])
        mn = min(mn, float(r["env_min"]))
        mx = max(mx, float(r["env_max"]))
        f |= int(r["flags"])
    if f:
        out["env_sum"], out["env_sq"], out["env_min"], out["env_max"] = s, q, mn, mx
        out["n"], out["flags"] = n, f
    return out


def _db(x: float) -> float:
    if x > 0.0:
        return 10.0 * math.log10(x)
    return -math.inf if x == 0.0 else math.nan


def status(row, ripple_max: float = RIPPLE_MAX) -> dict:
    """sdr_meter_rf_status in Python floats (IEEE double, the same operations in the same order)."""
    n = int(row["n"])
    m1 = float(row["env_sum"]) / n if n > 0 else 0.0
    m2 = float(row["env_sq"]) / n if n > 0 else 0.0
    zero = not (m1 != 0.0)
    out = {"level_dbfs": _db(m1), "ripple": 0.0 if zero else (m2 - m1 * m1) / (m1 * m1)}
    S = math.sqrt(max(2.0 * m1 * m1 - m2, 0.0))
    N = m1 - S
    if not S > 0.0:
        out["cnr_db"] = -math.inf
    elif N <= 0.0:
        out["cnr_db"] = math.inf
    else:
        out["cnr_db"] = 10.0 * math.log10(S / N)
    out["fade_db"] = 0.0 if zero else _db(float(row["env_min"]) / m1)
    out["crest_db"] = 0.0 if zero else _db(float(row["env_max"]) / m1)
    f = 0
    if (int(row["flags"]) & ROW_RF) and (zero or out["ripple"] > float(np.float32(ripple_max))):
        f |= WEAK
    out["flags"] = f
    return out


def _fmt(v: float) -> str:
    """A reading as PREFIX.rfstatus prints it (C's %.3f; the infinities as inf / -inf)."""
    if math.isinf(v):
        return "inf" if v > 0 else "-inf"
    return "%.3f" % v


def status_line(c: int, row) -> str:
    """The line of channel c in PREFIX.rfstatus, from its run-long row and the default options."""
    st = status(row)
    return ("ch %d: level_dbfs %s ripple %s cnr_db %s fade_db %s crest_db %s flags %s" %
            (c, _fmt(st["level_dbfs"]), _fmt(st["ripple"]), _fmt(st["cnr_db"]), _fmt(st["fade_db"]),
             _fmt(st["crest_db"]), "WEAK" if st["flags"] & WEAK else "-"))


def same_rows(got, want) -> list:
    """The fields in which two row arrays differ, floats compared as uint32: [] when equal."""
    got, want = np.asarray(got), np.asarray(want)
    bad = []
    for name in FLOAT_FIELDS:
        if not np.array_equal(np.ascontiguousarray(got[name]).view(np.uint32),
                              np.ascontiguousarray(want[name]).view(np.uint32)):
            bad.append(name)
    for name in ("n", "flags", "reserved"):
        if not np.array_equal(got[name], want[name]):
            bad.append(name)
    return bad


# ---------------------------------------------------------------- signals of the meaning tests
def carrier_noise_u8(n_iq: int, amp: float, sigma: float, seed: int, khz: float = 20.0, fs: float = 2.4e6):
    """u8 I/Q pairs [2 * n_iq]: an unmodulated carrier of amplitude `amp` at +khz plus complex Gaussian noise of
    `sigma` per component, as round(128 x + 128) clipped to u8 (the front end reads (u8 - 128) / 128)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_iq, dtype=np.float64)
    z = amp * np.exp(2j * np.pi * khz * 1e3 * t / fs)
    z = z + sigma * (rng.standard_normal(n_iq) + 1j * rng.standard_normal(n_iq))
    q = np.empty(2 * n_iq, np.float64)
    q[0::2] = np.round(128.0 * z.real + 128.0)
    q[1::2] = np.round(128.0 * z.imag + 128.0)
    return np.clip(q, 0, 255).astype(np.uint8)


def true_cnr_db(h, amp: float, sigma: float, khz: float = 20.0, fs: float = 2.4e6) -> float:
    """The in-channel C/N behind the taps h: the carrier's power through the filter's gain at its frequency over
    the white input noise (2 sigma^2 and the u8 rounding's 2 / (12 128^2)) through sum h^2."""
    h = np.asarray(h, np.float64)
    k = np.arange(h.size)
    gain = abs(np.sum(h * np.exp(-2j * np.pi * khz * 1e3 * k / fs))) ** 2
    noise = (2.0 * sigma * sigma + 2.0 / (12.0 * 128.0 * 128.0)) * float(np.sum(h * h))
    return 10.0 * math.log10(amp * amp * gain / noise)
