"""CPU model of the RDS carrier-phase derotator (include/sdr_amd.h, sdr_rds_carrier_*): the in-phase and
quadrature rows of the RDS chain are quantised once, the phase of the 57 kHz subcarrier against the chain's
carrier is estimated per window of the stream from the squared signal, and the rows are rotated onto one
axis. One quantisation, then all integer; k_rds_carrier must give the same output rows and stats for any cut
of a channel's stream into calls. The rules, in the header's words:

  qi, qq = rint(clamp(x * 2^qshift, +-32767)) (round to nearest even) of the two rows.
  y = clamp((qi c + qq s + 2^13) >> 14, +-32767), out = y * 2^-qshift (exact in f32): Re(z e^{-j phi}) with
    (c, s) = 2^14 (cos phi, sin phi), constant over a window of W = 2048 samples of the stream, (2^14, 0) in
    the first one.
  At the end of a window: Pr = sum(qi^2 - qq^2), Pi = sum(2 qi qq), Pt = sum(qi^2 + qq^2) over its samples,
    each at most W * 2^31 = 2^42 in magnitude; Sr += (Pr - Sr) >> avg_shift, Si and St likewise (arithmetic
    shift: S stays between its old value and P, so |S| <= 2^42 too).
  With m = max(|Sr|, |Si|) > 0: both are shifted by the same count, right (arithmetic) or left, that puts m
    into [2^28, 2^29); a vectoring CORDIC of N = 24 iterations gives the angle of (Sr, Si) as an int32 with a
    turn = 2^32; phi = angle >> 1, plus half a turn when |wrap32(phi - phi_prev)| > 2^30; a rotation CORDIC
    gives (c, s) for the next window. m = 0 keeps phi and (c, s).
  A call with a non-finite sample in either row writes an all-NaN output row and puts the channel back to its
    first window (phi = 0, S = 0; resets + 1, windows stays).
"""
from __future__ import annotations

import math

import numpy as np

W = 2048               # samples of the stream per window
QSHIFT = 10
AVG_SHIFT = 3          # k of S += (P - S) >> k
QMAX = 32767
ONE = 1 << 14          # Q14
N_CORDIC = 24
ATAN = (536870912, 316933406, 167458907, 85004756, 42667331, 21354465, 10679838, 5340245, 2670163, 1335087, 667544,
        333772, 166886, 83443, 41722, 20861, 10430, 5215, 2608, 1304, 652, 326, 163, 81)   # atan(2^-i), a turn = 2^32
X0 = 326016437         # 2^29 / prod sqrt(1 + 4^-i), i < 24
MAX_N = 19712          # SDR_RDS_TRACK_MAX_N: the rows go on to the tracker
I32 = (1 << 31) - 1
P_MAX = W << 31        # the bound of a window's sums and of S
STATS = ("sr", "si", "st", "phi", "windows", "resets", "reserved")
STATS_DTYPE = np.dtype([("sr", "<i8"), ("si", "<i8"), ("st", "<i8"), ("phi", "<i4"), ("windows", "<u4"),
                        ("resets", "<u4"), ("reserved", "<u4")])
DEFAULTS = dict(qshift=QSHIFT, avg_shift=AVG_SHIFT)

assert len(ATAN) == N_CORDIC and all(a == round(math.atan(2.0 ** -i) / (2 * math.pi) * 2 ** 32) for i, a in enumerate(ATAN))
assert X0 == round(2 ** 29 / math.prod(math.sqrt(1 + 4.0 ** -i) for i in range(N_CORDIC)))
# per sample: |qi^2 - qq^2| < 2^30, |2 qi qq| and qi^2 + qq^2 < 2^31: int32 products, int64 sums
assert 2 * QMAX * QMAX <= I32 and P_MAX == 1 << 42
# the rotation: |c| + |s| <= sqrt(2) * 2^14 + 2 (the CORDIC's error is below one unit each)
assert QMAX * (int(math.sqrt(2) * ONE) + 3) + (1 << 13) <= I32


def wrap32(v: int) -> int:
    return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def quantise(x, qshift: int = QSHIFT) -> np.ndarray:
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        y = np.clip(x * np.float32(1 << qshift), np.float32(-QMAX), np.float32(QMAX))
    return np.rint(y).astype(np.int64)


def normalise(sr: int, si: int) -> tuple:
    """The common shift that puts max(|sr|, |si|) > 0 into [2^28, 2^29)."""
    bl = max(abs(sr), abs(si)).bit_length()
    assert bl > 0
    if bl > 29:
        return sr >> (bl - 29), si >> (bl - 29)
    return sr << (29 - bl), si << (29 - bl)


def cordic_angle(x: int, y: int) -> int:
    """Vectoring: the angle of (x, y), |x|, |y| <= 2^29, as an int32 with a turn = 2^32."""
    assert abs(x) <= 1 << 29 and abs(y) <= 1 << 29
    z = 0
    if x < 0:
        x, y, z = -x, -y, 1 << 31
    for i, a in enumerate(ATAN):
        if y >= 0:
            x, y, z = x + (y >> i), y - (x >> i), z + a
        else:
            x, y, z = x - (y >> i), y + (x >> i), z - a
        assert abs(x) <= I32 and abs(y) <= I32
    return wrap32(z)


def cordic_vector(phi: int) -> tuple:
    """Rotation: (c, s) = 2^14 (cos phi, sin phi) of an int32 angle."""
    z, neg = int(phi), False
    if z > 1 << 30 or z < -(1 << 30):
        z, neg = wrap32(z - (1 << 31)), True
    x, y = X0, 0
    for i, a in enumerate(ATAN):
        if z >= 0:
            x, y, z = x - (y >> i), y + (x >> i), z - a
        else:
            x, y, z = x + (y >> i), y - (x >> i), z + a
        assert abs(x) <= I32 and abs(y) <= I32
    c, s = (x + (1 << 14)) >> 15, (y + (1 << 14)) >> 15
    return (-c, -s) if neg else (c, s)


class Channel:
    """One channel's derotator state."""

    def __init__(self, qshift: int = QSHIFT, avg_shift: int = AVG_SHIFT):
        if not 0 <= qshift <= 15 or not 0 <= avg_shift <= 6:
            raise ValueError("qshift 0..15, avg_shift 0..6")
        self.qshift, self.k = qshift, avg_shift
        self.reset()

    def reset(self):
        """sdr_rds_carrier_reset: everything, the counters included."""
        self.windows = self.resets = 0
        self._restart()

    def _restart(self):
        self.wcnt = 0                              # samples of the current window so far
        self.pr = self.pi = self.pt = 0
        self.sr = self.si = self.st = 0
        self.phi, self.c, self.s = 0, ONE, 0

    def _window(self):
        assert max(abs(self.pr), abs(self.pi), self.pt) <= P_MAX
        self.sr += (self.pr - self.sr) >> self.k
        self.si += (self.pi - self.si) >> self.k
        self.st += (self.pt - self.st) >> self.k
        assert max(abs(self.sr), abs(self.si), abs(self.st)) <= P_MAX
        self.pr = self.pi = self.pt = 0
        self.wcnt = 0
        self.windows += 1
        if self.sr == 0 and self.si == 0:
            return
        phi = cordic_angle(*normalise(self.sr, self.si)) >> 1
        if abs(wrap32(phi - self.phi)) > 1 << 30:
            phi = wrap32(phi + (1 << 31))
        self.phi = phi
        self.c, self.s = cordic_vector(phi)

    def call(self, xi, xq) -> np.ndarray:
        """One call of len(xi) == len(xq) samples: the output row, f32."""
        xi, xq = np.asarray(xi, np.float32), np.asarray(xq, np.float32)
        n = len(xi)
        assert len(xq) == n
        if n > MAX_N:
            raise ValueError(f"n {n} > {MAX_N}")
        if n == 0:
            return np.zeros(0, np.float32)
        if not (np.isfinite(xi).all() and np.isfinite(xq).all()):
            self.resets += 1
            self._restart()
            return np.full(n, np.nan, np.float32)
        qi, qq = quantise(xi, self.qshift), quantise(xq, self.qshift)
        y = np.empty(n, np.int64)
        a = 0
        while a < n:
            b = min(n, a + W - self.wcnt)
            i, q = qi[a:b], qq[a:b]
            acc = i * self.c + q * self.s + (1 << 13)
            assert np.abs(acc).max() <= I32
            y[a:b] = np.clip(acc >> 14, -QMAX, QMAX)
            self.pr += int(np.sum(i * i - q * q))
            self.pi += int(np.sum(2 * i * q))
            self.pt += int(np.sum(i * i + q * q))
            self.wcnt += b - a
            if self.wcnt == W:
                self._window()
            a = b
        self.y = y                                 # the integers behind the row, for the tests
        return y.astype(np.float32) * np.float32(2.0 ** -self.qshift)

    def stats(self) -> dict:
        return dict(sr=self.sr, si=self.si, st=self.st, phi=self.phi, windows=self.windows, resets=self.resets, reserved=0)

    def state(self) -> tuple:
        return (self.wcnt, self.pr, self.pi, self.pt, self.c, self.s) + tuple(self.stats()[k] for k in STATS)

    def phase_deg(self) -> float:
        return self.phi * 360.0 / 2.0 ** 32

    def coherence(self) -> float:
        return math.hypot(self.sr, self.si) / self.st if self.st else 0.0


def derotate(rows, **opts) -> tuple:
    """A stream given as an iterable of calls' (xi, xq): (the output rows concatenated, the Channel)."""
    ch = Channel(**opts)
    out = [ch.call(xi, xq) for xi, xq in rows]
    return (np.concatenate(out) if out else np.zeros(0, np.float32)), ch


# ------------------------------------------------------------------ test streams (no DSP)
def rotated(seed: int, n: int, deg, amp_q: int = 300, sigma_q: int = 120, qshift: int = QSHIFT) -> tuple:
    """(xi, xq, base): n samples of random biphase chips `base` (quantised units, as rds_track_model.chips at
    39 samples a chip) turned by `deg` degrees (a scalar or an array [n]) plus integer noise on both rows,
    rounded to multiples of 2^-qshift so that the quantisation is the identity on them."""
    rs = np.random.Generator(np.random.PCG64(seed))
    nchip = n // 39 + 2
    lvl = np.repeat(np.where(rs.integers(0, 2, nchip) > 0, amp_q, -amp_q), 39)[:n].astype(np.float64)
    th = np.deg2rad(np.broadcast_to(np.asarray(deg, np.float64), (n,)))
    i = np.rint(lvl * np.cos(th)) + rs.integers(-sigma_q, sigma_q + 1, n)
    q = np.rint(lvl * np.sin(th)) + rs.integers(-sigma_q, sigma_q + 1, n)
    k = np.float32(2.0 ** -qshift)
    return i.astype(np.float32) * k, q.astype(np.float32) * k, lvl


OFF_GRID_SPECIALS = (3e38, -3e38, 1e-40, -0.0, 32.0, 31.9985, -32.0)   # the last three in units of 2^(QSHIFT - qshift)


def off_grid(seed: int, n: int, deg: float, qshift: int = QSHIFT, gain: float = 1.0) -> tuple:
    """(xi, xq) that the quantisation has to round: rotated() times f32 factors from [0.9, 1.1] (and `gain`: a
    large one drives both rows into the clamp), with exact ties (k + 0.5) * 2^-qshift of both signs and
    OFF_GRID_SPECIALS sprinkled over both rows: products that overflow before the clamp, a subnormal, -0.0, the
    clamp's bounds and the last value below one."""
    rs = np.random.Generator(np.random.PCG64(seed))
    out = []
    xi, xq, _ = rotated(seed, n, deg, qshift=qshift)
    for x in (xi, xq):
        x = x * rs.uniform(0.9, 1.1, n).astype(np.float32) * np.float32(gain)
        nties = max(16, n // 40)
        special = np.array(OFF_GRID_SPECIALS, np.float32)
        special[4:] *= np.float32(2.0 ** (QSHIFT - qshift))
        if n >= 2 * (nties + len(special)):
            at = rs.permutation(n)[:nties + len(special)]
            kk = rs.integers(-400, 400, nties).astype(np.float32)
            x[at[:nties]] = (kk + np.float32(0.5)) * np.float32(2.0 ** -qshift)
            x[at[nties:]] = special
        out.append(x.astype(np.float32))
    return out[0], out[1]
