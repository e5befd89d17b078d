"""CPU model of the RDS soft decisions (include/sdr_amd.h, sdr_rds_track_bits_soft and sdr_rds_*_soft): the
symbol tracker's per-bit reliabilities and the group decoder's Chase step over the least reliable raw
decisions of a failing block. All integer; the kernels must give the same soft rows, group records, counters
and reliability history for any cut of a channel's stream into calls. It adds to tests/rds_track_model.py and
tests/rds_model.py and changes neither. The rules, in the header's words:

  Tracker: the bit decided at t also gets soft = |c(t)| >> 6 as u16 (78 * 32767 >> 6 = 39934: no clamp).
    soft[k] belongs to raw decision k; bit k = raw k ^ raw k-1 as before. The clock, the bits, nbits, the
    stats and the poisoning are those of rds_track_model.Channel; a poisoned call writes no soft values.
  Decoder: soft_bits = L in 0..6; L = 0 is rds_model.Channel bit for bit. The decoder keeps the reliabilities
    of the last HIST = 32 bits it consumed. At a judgement at bit i, between step 3 (late) and step 4 (the
    burst table), on the nominal word (diff bits i-26 .. i-1, the first in bit 25) only:
      candidates  the 27 raw decisions i-27 .. i-1 stand behind those diff bits (window position p = 0..26 is
                  raw i-27+p); the candidates are the L of them with the smallest (soft, p): older first on ties
      patterns    m = 1 .. 2^L-1 flips the candidates whose bit is set in m, bit j of m being the j-th
                  candidate in that order. A flipped raw r toggles diff bits r and r+1, clipped to the window:
                  toggle(p) = ((3 << 26) >> (p + 1)) & M26, one bit for p = 0 and p = 26. e(m) is their XOR; any
                  26 of the 27 toggles are linearly independent, so e(m) != 0 for L <= 6 < 27 (asserted).
      weight      w(m) = the sum of the flipped candidates' soft, at most 6 * 65535 < 2^19 (6 * 39934 < 2^18
                  for the tracker's softs)
      acceptance  of all m whose nominal ^ e(m) matches an offset of block expect (C before C'), the smallest
                  (w, m) wins
      effect      the word is placed as corrected, exactly like step 4: its bit goes into ok and corrected,
                  corrected + 1, bad_run stays, next judgement at i + 26; its bit also goes into the soft mask,
                  the high nibble of the group's flags (GROUP_SOFT_SHIFT = 4); reserved stays 0.
                  soft_blocks + 1, soft_flips + popcount(m)
      fallback    no m matches: steps 4 and 5 as before
    A call: -1 and invalid nbits consume nothing, soft values included. NBITS_POISONED is rds_model's (the
    history stays as it is). No judgement window reaches across a poisoned call, a loss of sync or the reset:
    each leaves the channel not synchronised with no pending hit; sync then needs a pending hit behind the
    break and a second hit at a bit i at least 26 bits later, and the first judgement is at i + 27 with the
    window i .. i + 26. Every later window begins at least 25 bits further on. So every soft in a window
    belongs to a bit consumed after the break, and the first judgement after a reset is at bit
    FIRST_JUDGEMENT = 25 + 26 + 27 = 78 or later.
"""
from __future__ import annotations

import numpy as np

import rds_model as rm
import rds_track_model as tm

HIST = 32
MAX_SOFT_BITS = 6
GROUP_SOFT_SHIFT = 4
SOFT_MAX = (tm.B * tm.QMAX) >> 6               # 39934
SOFT_DEFAULTS = dict(max_burst=2, loss_blocks=8, soft_bits=6)
SOFT_COUNTERS = ("soft_blocks", "soft_flips")
SOFT_STATS_DTYPE = np.dtype([("soft_blocks", "<u4"), ("soft_flips", "<u4"), ("soft_bits", "<u4"), ("reserved", "<u4")])
FIRST_JUDGEMENT = 25 + 26 + 27                 # the earliest bit index of a judgement after a reset

assert SOFT_MAX == 39934 and MAX_SOFT_BITS * SOFT_MAX < 1 << 18 and MAX_SOFT_BITS * 65535 < 1 << 19


def toggle(p: int) -> int:
    """The diff bits of the nominal word that flipping window raw p (0 = the oldest of the 27) toggles."""
    return ((3 << 26) >> (p + 1)) & rm.M26


# ------------------------------------------------------------------ the tracker
class TrackChannel(tm.Channel):
    """rds_track_model.Channel whose call also returns the reliabilities: (nbits, bits, soft). The body is the
    parent's call with one line more at the decision; tests/test_rds_soft_model.py holds the two together."""

    def call(self, x):
        x = np.asarray(x, np.float32)
        n = len(x)
        if n > tm.MAX_N:
            raise ValueError(f"n {n} > {tm.MAX_N}")
        if n and not np.isfinite(x).all():
            self.resets += 1
            self._restart()
            return tm.NBITS_POISONED, [], []
        if n == 0:
            return 0, [], []
        S, B, T = tm.S, tm.B, tm.T
        buf = np.concatenate([self.carry, tm.quantise(x, self.qshift)])
        P = np.concatenate([[0], np.cumsum(buf)])
        base = self.n - tm.CARRY
        n1 = self.n + n

        def c(t):
            j = t - base
            return 2 * P[j + S] - P[j] - P[j + B]

        A, H = self.A, self.H
        out: list = []
        soft: list = []
        if not self.locked:
            hi = min(n1 - B, A * B - 1)
            if hi >= self.ta:
                ts = np.arange(self.ta, hi + 1)
                np.add.at(self.E, ts % B, np.abs(c(ts)))
                self.ta = hi + 1
            if self.ta == A * B:
                self.locked = 1
                self.acquired += 1
                self.t = A * B + int(np.argmax(self.E))
        if self.locked:
            while self.t + B + 1 <= n1:
                t = self.t
                on = int(c(t))
                raw = 1 if on > 0 else 0
                out.append(raw ^ self.prev)
                soft.append(abs(on) >> 6)
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
        assert len(out) <= tm.MAX_BITS and all(0 <= v <= SOFT_MAX for v in soft)
        self.bits += len(out)
        self.carry = buf[-tm.CARRY:].copy()
        self.n = n1
        return len(out), out, soft


def track_soft(rows, **opts) -> tuple:
    """A stream given as an iterable of calls' rows: (bits, softs, the TrackChannel)."""
    ch = TrackChannel(**opts)
    bits: list = []
    soft: list = []
    for x in rows:
        nb, b, s = ch.call(x)
        if nb > 0:
            bits += b
            soft += s
    return bits, soft, ch


# ------------------------------------------------------------------ the decoder
class Channel(rm.Channel):
    """rds_model.Channel with the soft step. bit(b, soft, out) and call(nbits, bits, soft)."""

    def __init__(self, max_burst: int = 2, loss_blocks: int = 8, soft_bits: int = 6):
        if not 0 <= soft_bits <= MAX_SOFT_BITS:
            raise ValueError("soft_bits 0..6")
        self.soft_bits = soft_bits
        super().__init__(max_burst, loss_blocks)

    def reset(self):
        super().reset()
        self.hist = [0] * HIST                     # the softs of the last HIST bits consumed, the newest last
        self.soft_blocks = self.soft_flips = 0
        self.last_win = None                       # (w, m, e) of the last soft correction, for the tests

    def soft_search(self, nominal: int, window, expect: int):
        """The winner (w, m, e, offset) over the 27 window softs (oldest first), or None."""
        assert len(window) == 27
        order = sorted(range(27), key=lambda p: (window[p], p))[:self.soft_bits]
        best = None
        for m in range(1, 1 << self.soft_bits):
            e = w = 0
            for j, p in enumerate(order):
                if (m >> j) & 1:
                    e ^= toggle(p)
                    w += window[p]
            assert e != 0, "fewer than 27 toggles are independent"
            o = self._match(nominal ^ e, expect)
            if o >= 0 and (best is None or (w, m) < best[:2]):
                best = (w, m, e, o)
        return best

    def bit(self, b: int, soft: int, out: list):            # noqa: C901 -- rds_model.Channel.bit with one step more
        i = self.n
        self.hist = self.hist[1:] + [int(soft)]
        if not self.synced or i != self.judge_at:
            return super().bit(b, out)
        assert i >= FIRST_JUDGEMENT
        sr = ((self.sr << 1) | (b & 1)) & rm.M64
        nominal = (sr >> 1) & rm.M26
        hit = any(self._match(w, self.expect) >= 0 for w in (nominal, (sr >> 2) & rm.M26, sr & rm.M26))
        win = None if hit or not self.soft_bits else self.soft_search(nominal, self.hist[-28:-1], self.expect)
        if win is None:
            return super().bit(b, out)                     # steps 1-3, or 4 and 5
        w, m, e, o = win
        self.sr = sr
        self.n += 1
        self.corrected += 1
        self.soft_blocks += 1
        self.soft_flips += bin(m).count("1")
        self.last_win = (w, m, e)
        self.flags |= 1 << (GROUP_SOFT_SHIFT + self.expect)
        self._place(nominal ^ e, o, corrected=True)
        self.judge_at = i + 26
        self._end_of_block(out)

    def call(self, nbits: int, bits, soft=None) -> list:
        out: list = []
        if nbits == rm.NBITS_POISONED:
            return super().call(nbits, bits)
        if nbits < 0 or nbits > rm.MAX_BITS:
            return out
        for k in range(nbits):
            self.bit(int(bits[k]), int(soft[k]) if soft is not None else 0, out)
        assert len(out) <= rm.MAX_GROUPS
        return out

    def soft_stats(self) -> dict:
        return dict(soft_blocks=self.soft_blocks, soft_flips=self.soft_flips, soft_bits=self.soft_bits, reserved=0)

    def state(self) -> tuple:
        return super().state() + (tuple(self.hist), self.soft_blocks, self.soft_flips)


def decode(bits, soft, **opts):
    """A whole stream through one channel: (group tuples, Channel)."""
    ch = Channel(**opts)
    out: list = []
    for b, s in zip(bits, soft):
        ch.bit(int(b), int(s), out)
    return out, ch


def group_line(ch: int, g) -> str:
    """The PREFIX.groups line of a group tuple: a soft-corrected block ends in '~', a burst-corrected one in '*'."""
    f = []
    for b in range(4):
        if not (g[1] >> b) & 1:
            f.append("----")
        else:
            mark = "~" if (g[3] >> (GROUP_SOFT_SHIFT + b)) & 1 else "*" if (g[2] >> b) & 1 else ""
            f.append("%04X%s" % (g[0][b], mark))
    return "ch %d bits %d %s" % (ch, g[5], " ".join(f))


# ------------------------------------------------------------------ test streams (no DSP)
def random_softs(streams, seed: int = 11) -> list:
    """A u16 soft per bit of every stream: mostly mid-range values, ties, zeros and 65535 sprinkled in."""
    rs = np.random.Generator(np.random.PCG64(seed))
    out = []
    for s in streams:
        v = rs.integers(0, 4000, len(s))
        v[rs.random(len(s)) < 0.2] = 1000                   # ties
        v[rs.random(len(s)) < 0.02] = 0
        v[rs.random(len(s)) < 0.02] = 65535
        out.append([int(x) for x in v])
    return out


def raw_errors(bits, at) -> list:
    """bits (diff bits) after flipping the raw decisions at the indices `at`: raw r toggles diff bits r and r+1."""
    out = list(bits)
    for r in at:
        for k in (r, r + 1):
            if 0 <= k < len(out):
                out[k] ^= 1
    return out


def noisy_chips(bits, seed: int, amp_q: int = 300, noise_q: int = 2500) -> np.ndarray:
    """rds_track_model.chips of a bit list at amplitude amp_q with uniform integer noise +-noise_q, in exact
    multiples of 2^-QSHIFT."""
    rs = np.random.Generator(np.random.PCG64(seed))
    x = tm.chips(bits, float(amp_q))
    x = x + rs.integers(-noise_q, noise_q + 1, len(x)).astype(np.float32)
    return (x / np.float32(1 << tm.QSHIFT)).astype(np.float32)


def make_soft_streams(synth, nbits: int = 3016, seed: int = 23):
    """(streams, softs): rds_model.make_streams' eight streams with random_softs, and in every third block of
    each 1 to 7 raw decisions flipped and given the block's lowest soft values, so that the soft step runs,
    wins with every popcount up to 6 and fails (7 flips) in every stream that holds groups."""
    rs = np.random.Generator(np.random.PCG64(seed))
    streams = [list(s) for s in rm.make_streams(synth, nbits)]
    softs = random_softs(streams, seed + 1)
    for c, s in enumerate(streams):
        for blk in range(2, len(s) // 26 - 1, 3):
            k = 1 + (blk // 3 + c) % 7
            at = sorted(int(v) for v in rs.choice(27, k, replace=False))
            raws = [26 * blk - 1 + p for p in at]
            s[:] = raw_errors(s, raws)
            lo = 26 * blk - 1
            for r in range(lo, lo + 27):                        # the block's other raws are well above
                softs[c][r] = max(softs[c][r], 100) if softs[c][r] != 65535 else 65535
            for j, r in enumerate(raws):
                softs[c][r] = int(rs.integers(0, 3)) + (j if k > 3 else 0)
    return streams, softs


# ------------------------------------------------------------------ hand-built cases
BLOCK = 4 * 2 + 1            # the block the hand-built cases damage: group 2, block B
HI = 1000                    # the soft of an undamaged raw in them
SEVEN = (2, 1, 6, 11, 8, 13, 17)      # window positions of which no subset's toggles make a code word


def damaged(clean_bits, flips: dict, block: int = BLOCK, others: int = HI):
    """(bits, soft) of a clean stream that starts on a group boundary (block k is bits 26 k .. 26 k + 25, judged
    at i = 26 (k + 1) with the window raws 26 k - 1 .. 26 k + 25): raw errors at the window positions of `flips`
    (position -> soft) of `block`; a position mapped to (soft, False) gets the soft value without an error."""
    soft = [others] * len(clean_bits)
    at = []
    for p, v in flips.items():
        v, err = v if isinstance(v, tuple) else (v, True)
        soft[26 * block - 1 + p] = v
        if err:
            at.append(26 * block - 1 + p)
    return raw_errors(clean_bits, at), soft


def toggle_sets(target: int, size: int = 4):
    """Sets of `size` window positions, no edge raw among them, whose toggles XOR to a word of syndrome `target`."""
    import itertools
    for D in itertools.combinations(range(1, 26), size):
        e = 0
        for p in D:
            e ^= toggle(p)
        if rm.syndrome(e) == target:
            yield D, e


def hand_built_cases(clean_bits, nbits: int = 26 * 16) -> list:
    """[(name, bits, soft)]: the cases of tests/test_rds_soft_model.py on the first nbits of the clean stream, for
    a decoder to be run on at any soft_bits."""
    cb = clean_bits[:nbits]
    cases = [("raw %d" % p, *damaged(cb, {p: 5})) for p in range(27)]
    for k in range(1, 8):
        cases.append(("%d errors" % k, *damaged(cb, {p: j + 1 for j, p in enumerate(SEVEN[:k])})))
    quiet = {2: (1, False), 1: (2, False), 6: (3, False), 11: (4, False), 8: (5, False), 17: (6, False)}
    cases.append(("seventh", *damaged(cb, {**quiet, 13: 7})))
    cases.append(("tie", *damaged(cb, {**quiet, 13: 6})))
    for level in (0, 1000, 65535):
        cases.append(("equal %d" % level, *damaged(cb, {p: level for p in range(1, 6)}, others=level)))
        cases.append(("equal %d out" % level, *damaged(cb, {6: level}, others=level)))
    D, _ = next(toggle_sets(rm.OFFSET_WORDS[2] ^ rm.OFFSET_WORDS[3]))
    for softs in ((1, 2, 3, 4), (3, 4, 1, 2), (2, 3, 1, 4)):
        flips = {D[0]: softs[0], D[1]: softs[1], D[2]: (softs[2], False), D[3]: (softs[3], False)}
        cases.append(("c/c' %s" % (softs,), *damaged(cb, flips, block=4 * 2 + 2)))
    D, _ = next(toggle_sets(0))
    cases.append(("soft before burst", *damaged(cb, {D[0]: 900, D[1]: (1, False), D[2]: (2, False), D[3]: (3, False)})))
    return cases
