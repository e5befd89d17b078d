"""CPU model of the RDS symbol tracker (include/sdr_amd.h, sdr_rds_track_*): a biphase correlator over the
whole bit on a bit clock that is carried across calls and nudged by early/late sums. One quantisation,
then all integer; k_rds_track must give the same nbits, bits and stats for any cut of a channel's stream
into calls. The rules, in the header's words:

  q = rint(clamp(x * 2^QSHIFT, +-32767)) (round to nearest even), int32; a call with a non-finite sample
  gives NBITS_POISONED and puts the channel back to acquiring with an empty stream.
  c(t) = sum q[t .. t+S-1] - sum q[t+S .. t+B-1], t the index in the stream since the last reset.
  Acquiring: every t < A * B adds |c(t)| to E[t mod B] once sample t + B - 1 is in; after t = A * B - 1
    the first maximum of E is the phase and the first bit starts at t = A * B + phase.
  Tracking: the bit at t is decided once sample t + B is in: raw = c(t) > 0, out = raw ^ previous raw,
    t += B. Its |c(t-1)|, |c(t)|, |c(t+1)|, |c(t-S)| go to the sums early, on, late, half; after T bits
    level = on, the last four go to the half check's on and half sums, and then, the first that holds:
      the H / T-th such round and half sum > on sum:  t += S, half_moves + 1
      early > on and early >= late:                   t -= 1, moves + 1
      late > on:                                      t += 1, moves + 1
    (the half check's sums start again after its H bits, the others after every T).
  |c(t-S)| is the half-bit correlator c(t'+S) of the bit before, t' = t - B: it ends S - 1 samples after
  that bit's own decision point, so it is taken one bit late, from samples that are all in.
"""
from __future__ import annotations

import numpy as np

S = 39                 # samples per chip in mode 0 (symbol_Fs)
B = 2 * S              # samples per bit
QSHIFT = 10
QMAX = 32767
A = 32                 # bit periods of acquisition
T = 16                 # bits per early/late decision
H = 64                 # bits per half-bit check
CARRY = 120            # quantised samples kept between calls: B + S + 1 are needed, 120 is the next multiple of 8
MAX_BITS = 256
MAX_N = (MAX_BITS - 1) * (B - 1) + B - 1       # 19712: bits are at least B - 1 samples apart
NBITS_POISONED = -2
I32 = (1 << 31) - 1
STATS = ("locked", "phase", "bits", "moves", "half_moves", "resets", "level", "acquired")
STATS_DTYPE = np.dtype([(n, "<u4") for n in STATS])

assert H % T == 0 and CARRY >= B + S + 1
# the int32 bounds: a call's prefix sums, the correlator, and each accumulator at its longest
assert (CARRY + MAX_N) * QMAX <= I32
assert B * QMAX * 64 <= I32                      # A and H are at most 64


DEFAULTS = dict(qshift=QSHIFT, acquire_bits=A, half_bits=H)


def quantise(x, qshift: int = QSHIFT) -> np.ndarray:
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        y = np.clip(x * np.float32(1 << qshift), np.float32(-QMAX), np.float32(QMAX))
    return np.rint(y).astype(np.int64)


class Channel:
    """One channel's tracker state."""

    def __init__(self, qshift: int = QSHIFT, acquire_bits: int = A, half_bits: int = H):
        if not 0 <= qshift <= 15 or not 1 <= acquire_bits <= 64 or not T <= half_bits <= 64 or half_bits % T:
            raise ValueError("qshift 0..15, acquire_bits 1..64, half_bits a multiple of T in T..64")
        self.qshift, self.A, self.H = qshift, acquire_bits, half_bits
        self.reset()

    def reset(self):
        """sdr_rds_track_reset: everything, the counters included."""
        self.bits = self.moves = self.half_moves = self.resets = self.acquired = 0
        self._restart()

    def _restart(self):
        self.n = 0                                 # samples consumed since the stream (re)started
        self.carry = np.zeros(CARRY, np.int64)
        self.locked = 0
        self.E = np.zeros(B, np.int64)
        self.ta = 0                                # the next position acquisition adds
        self.t = 0                                 # the next bit's start
        self.prev = 0
        self.cnt = 0
        self.early = self.on = self.late = self.half = 0
        self.hr = 0
        self.hon = self.hhalf = 0
        self.level = 0

    def call(self, x):
        """One call of len(x) samples: (nbits, the bits as a list)."""
        x = np.asarray(x, np.float32)
        n = len(x)
        if n > MAX_N:
            raise ValueError(f"n {n} > {MAX_N}")
        if n and not np.isfinite(x).all():
            self.resets += 1
            self._restart()
            return NBITS_POISONED, []
        if n == 0:
            return 0, []
        buf = np.concatenate([self.carry, quantise(x, self.qshift)])
        P = np.concatenate([[0], np.cumsum(buf)])
        assert np.abs(P).max() <= I32
        base = self.n - CARRY                      # the stream index of buf[0]
        n1 = self.n + n

        def c(t):
            j = t - base
            assert np.min(j) >= 0 and np.max(j) + B <= len(buf)
            v = 2 * P[j + S] - P[j] - P[j + B]
            assert np.max(np.abs(v)) <= B * QMAX
            return v

        A, H = self.A, self.H
        out: list = []
        if not self.locked:
            hi = min(n1 - B, A * B - 1)
            if hi >= self.ta:
                ts = np.arange(self.ta, hi + 1)
                np.add.at(self.E, ts % B, np.abs(c(ts)))
                assert self.E.max() <= I32
                self.ta = hi + 1
            if self.ta == A * B:
                self.locked = 1
                self.acquired += 1
                self.t = A * B + int(np.argmax(self.E))          # argmax: the first maximum
        if self.locked:
            while self.t + B + 1 <= n1:
                t = self.t
                on = int(c(t))
                raw = 1 if on > 0 else 0
                out.append(raw ^ self.prev)
                self.prev = raw
                self.early += abs(int(c(t - 1)))
                self.on += abs(on)
                self.late += abs(int(c(t + 1)))
                self.half += abs(int(c(t - S)))
                self.cnt += 1
                self.t += B
                if self.cnt < T:
                    continue
                self.level = self.on
                self.hon += self.on
                self.hhalf += self.half
                self.hr += 1
                assert max(self.early, self.on, self.late, self.half, self.hon, self.hhalf) <= I32
                jump = False
                if self.hr == H // T:
                    jump = self.hhalf > self.hon
                    self.hr = self.hon = self.hhalf = 0
                if jump:
                    self.t += S
                    self.half_moves += 1
                elif self.early > self.on and self.early >= self.late:
                    self.t -= 1
                    self.moves += 1
                elif self.late > self.on:
                    self.t += 1
                    self.moves += 1
                self.cnt = 0
                self.early = self.on = self.late = self.half = 0
        assert len(out) <= MAX_BITS
        self.bits += len(out)
        self.carry = buf[-CARRY:].copy()
        self.n = n1
        return len(out), out

    def stats(self) -> dict:
        return dict(locked=self.locked, phase=self.t % B if self.locked else 0, bits=self.bits & 0xFFFFFFFF,
                    moves=self.moves, half_moves=self.half_moves, resets=self.resets, level=self.level,
                    acquired=self.acquired)

    def state(self) -> tuple:
        return (self.n, tuple(int(v) for v in self.carry), self.locked, tuple(int(v) for v in self.E), self.ta, self.t,
                self.prev, self.cnt, self.early, self.on, self.late, self.half, self.hr, self.hon, self.hhalf) + \
            tuple(self.stats()[k] for k in STATS)


def track(rows, **opts) -> tuple:
    """A stream given as an iterable of calls' rows: (all bits as a list, the Channel)."""
    ch = Channel(**opts)
    out: list = []
    for x in rows:
        nb, bits = ch.call(x)
        if nb > 0:
            out += bits
    return out, ch


# ------------------------------------------------------------------ test streams (no DSP)
def chips(bits, amp: float = 1.0, first: int = 0) -> np.ndarray:
    """Differentially encoded biphase chips of a bit list at S samples a chip, as f32: bit b toggles the
    level d (d ^= b), and a level is the chip pair (+a, -a) for 1 and (-a, +a) for 0."""
    d, out = first, np.empty(len(bits) * B, np.float32)
    for k, b in enumerate(bits):
        d ^= int(b) & 1
        v = amp if d else -amp
        out[k * B:k * B + S] = v
        out[k * B + S:(k + 1) * B] = -v
    return out


def noise_rows(seed: int, n: int, amp_q: int = 300, sigma_q: int = 200) -> tuple:
    """(x, bits): n samples of random bits' chips plus integer noise, in exact multiples of 2^-QSHIFT, so the
    quantisation is the identity on them."""
    rs = np.random.Generator(np.random.PCG64(seed))
    nb = n // B + 2
    bits = rs.integers(0, 2, nb)
    x = chips(bits, float(amp_q))[:n] + rs.integers(-sigma_q, sigma_q + 1, n).astype(np.float32)
    return (x / np.float32(1 << QSHIFT)).astype(np.float32), [int(b) for b in bits]


def for_qshift(x, qshift: int) -> np.ndarray:
    """x, made for QSHIFT, scaled by the power of two that gives the same x * 2^qshift (exact in f32 for the
    samples of noise_rows and wrong_half; off_grid takes qshift itself, its +-3e38 would overflow here)."""
    return (np.asarray(x, np.float32) * np.float32(2.0 ** (QSHIFT - qshift))).astype(np.float32)


OFF_GRID_SPECIALS = (3e38, -3e38, 1e-40, -0.0, 32.0, 31.9985)   # 32.0 and 31.9985 are in units of 2^(QSHIFT - qshift)


def off_grid(seed: int, n: int, qshift: int = QSHIFT, amp_q: int = 300, sigma_q: int = 200, gain: float = 1.0,
             quiet_tail: int = 0) -> np.ndarray:
    """n samples that the quantisation has to round: noise_rows times f32 factors drawn from [0.9, 1.1] (and
    `gain`), then, everywhere but in the last quiet_tail samples, a sprinkling of exact ties (k + 0.5) * 2^-qshift
    of both signs, and OFF_GRID_SPECIALS four times each: products that overflow before the clamp, a subnormal,
    -0.0, the clamp's bound and the last value below it. For another qshift the same quantised stream."""
    rs = np.random.Generator(np.random.PCG64(seed))
    x = noise_rows(seed, n, amp_q, sigma_q)[0] * rs.uniform(0.9, 1.1, n).astype(np.float32) * np.float32(gain)
    x = for_qshift(x, qshift)
    nties = max(64, n // 40)
    at = rs.permutation(n - quiet_tail)[:nties + 4 * len(OFF_GRID_SPECIALS)]
    assert len(at) == nties + 4 * len(OFF_GRID_SPECIALS), "off_grid: n is too small for its sprinkling"
    k = rs.integers(-400, 400, nties).astype(np.float32)                     # k + 0.5: -399.5 .. 399.5
    x[at[:nties]] = (k + np.float32(0.5)) / np.float32(1 << qshift)
    special = np.array(OFF_GRID_SPECIALS, np.float32)
    special[4:] = for_qshift(special[4:], qshift)
    x[at[nties:]] = np.tile(special, 4)
    return x


def walking(seed: int, n: int, every: int, doubled: bool, amp_q: int = 300, sigma_q: int = 200) -> np.ndarray:
    """n samples of noise_rows with one sample in every `every` deleted (or doubled): at every = 16 B - 1
    deleted the clock steps early each round of T bits, at 16 B + 1 doubled it steps late each round."""
    steps = n // every
    x = noise_rows(seed, n + steps, amp_q, sigma_q)[0]
    at = np.arange(1, steps + 1) * every - 1
    return (np.insert(x, at, x[at]) if doubled else np.delete(x, at))[:n]


CHUNK = 3072                                   # k_rds_track stages a call in chunks of this many samples (TRK_CHUNK)
BOUNDARY_SIZES = (0, 1, 2, 3, 4, 5, CARRY - 1, CARRY, CARRY + 1, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 3, 2 * CHUNK,
                  2 * CHUNK + 1, MAX_N - 1, MAX_N)


def boundary_plan(seed: int, ncalls: int = 40) -> list:
    """Call lengths at the kernel's edges: every one of BOUNDARY_SIZES once and further ones of at most two
    chunks and a sample, in a seeded order."""
    rs = np.random.Generator(np.random.PCG64(seed))
    small = [n for n in BOUNDARY_SIZES if n <= 2 * CHUNK + 1]
    plan = list(BOUNDARY_SIZES) + [int(v) for v in rs.choice(small, ncalls - len(BOUNDARY_SIZES))]
    plan = [plan[i] for i in rs.permutation(len(plan))]
    assert set(plan) == set(BOUNDARY_SIZES) and len(plan) == ncalls
    return plan


def wrong_half(seed: int, n: int, acquire_bits: int = A, amp_q: int = 300, sigma_q: int = 150) -> np.ndarray:
    """n samples whose acquisition takes the wrong half: acquire_bits + 4 zero bits without noise (the two
    alignments are then equal and the first maximum is the smaller residue), then noisy data; the right phase
    is 50, acquisition takes 50 - S = 11."""
    rs = np.random.Generator(np.random.PCG64(seed))
    bits = [0] * (acquire_bits + 4) + [int(v) for v in rs.integers(0, 2, n // B + 3)]
    x = chips(bits, float(amp_q))[(-50) % B:][:n]
    quiet = (acquire_bits + 3) * B
    x[quiet:] += rs.integers(-sigma_q, sigma_q + 1, max(n - quiet, 0)).astype(np.float32)
    return (x / np.float32(1 << QSHIFT)).astype(np.float32)
