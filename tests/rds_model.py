"""CPU model of the RDS group decoder (include/sdr_amd.h, sdr_rds_*): block synchronisation with a
flywheel, +-1 bit slip recovery and burst-error correction, one bit at a time. All integer; k_rds_groups
must give the same group records, counters and state for any split of a channel's bits into calls.
Also the text layer's field rules, restated for the tests (station_*)."""
from __future__ import annotations

import numpy as np

POLY = 0x5B9                       # g(x) = x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
OFFSET_WORDS = (0x0FC, 0x198, 0x168, 0x350, 0x1B4)      # A, B, C, C', D
OFFSET_BLOCK = (0, 1, 2, 2, 3)
BLOCK_OFFSETS = ((0,), (1,), (2, 3), (4,))              # the offsets of a block index, in trial order
M26 = (1 << 26) - 1
M64 = (1 << 64) - 1
MAX_GROUPS = 4
MAX_BITS = 256
NBITS_NONE = -1
NBITS_POISONED = -2
DEFAULTS = dict(max_burst=2, loss_blocks=8)

GROUP_DTYPE = np.dtype([("w", "<u2", (4,)), ("ok", "u1"), ("corrected", "u1"), ("flags", "u1"), ("reserved", "u1"),
                        ("bits", "<u4")])
COUNTERS = ("good", "corrected", "bad", "slips", "acquired", "lost", "groups")


def syndrome(w26: int) -> int:
    """The remainder of the 26-bit word (first bit received = bit 25) modulo g(x)."""
    reg = w26 & M26
    for bit in range(25, 9, -1):
        if reg & (1 << bit):
            reg ^= POLY << (bit - 10)
    return reg & 0x3FF


def parity_rows():
    """Row r of the parity-check matrix as a 26-bit mask: syndrome bit r = parity(w26 & row[r])."""
    rows = [0] * 10
    for k in range(26):
        s = syndrome(1 << k)
        for r in range(10):
            if (s >> r) & 1:
                rows[r] |= 1 << k
    return rows


def burst_patterns(max_burst: int):
    """Every non-zero error pattern whose set bits span at most max_burst positions of the 26."""
    out = []
    for length in range(1, max_burst + 1):
        inner = [0] if length == 1 else range(1 << (length - 2))
        for mid in inner:
            p = 1 if length == 1 else (1 << (length - 1)) | (mid << 1) | 1
            for pos in range(0, 26 - length + 1):
                out.append(p << pos)
    return out


def correction_table(max_burst: int):
    """(tab[1024], entries): tab[syndrome(e)] = e for every burst pattern e, 0 where not correctable."""
    if not 0 <= max_burst <= 5:
        raise ValueError("max_burst: 0..5")
    tab = np.zeros(1024, np.uint32)
    n = 0
    for e in burst_patterns(max_burst):
        s = syndrome(e)
        assert s != 0 and tab[s] == 0, "burst syndromes are distinct and non-zero up to length 5"
        tab[s] = e
        n += 1
    return tab, n


class Channel:
    """One channel's decoder state."""

    def __init__(self, max_burst: int = 2, loss_blocks: int = 8):
        if not 0 <= max_burst <= 5 or not 1 <= loss_blocks <= 64:
            raise ValueError("max_burst 0..5, loss_blocks 1..64")
        self.tab = [int(v) for v in correction_table(max_burst)[0]]
        self.loss_blocks = loss_blocks
        self.reset()

    def reset(self):
        self.sr = 0
        self.n = 0
        self.synced = 0
        self.expect = 0
        self.judge_at = 0
        self.bad_run = 0
        self.pending = None
        self._clear_assembly()
        for c in COUNTERS:
            setattr(self, c, 0)

    def _clear_assembly(self):
        self.w = [0, 0, 0, 0]
        self.ok = 0
        self.cmask = 0
        self.flags = 0

    def _place(self, word26: int, off: int, corrected: bool = False):
        b = self.expect
        self.w[b] = (word26 >> 10) & 0xFFFF
        self.ok |= 1 << b
        if corrected:
            self.cmask |= 1 << b
        if off == 3:
            self.flags |= 1

    def _end_of_block(self, out):
        if self.expect == 3:
            if self.ok:
                self.groups += 1
                out.append((tuple(self.w), self.ok, self.cmask, self.flags, 0, self.n & 0xFFFFFFFF))
            self._clear_assembly()
        self.expect = (self.expect + 1) & 3

    def _lose(self):
        self.synced = 0
        self.lost += 1
        self.pending = None
        self._clear_assembly()

    def _match(self, word26: int, block: int):
        s = syndrome(word26)
        for o in BLOCK_OFFSETS[block]:
            if s == OFFSET_WORDS[o]:
                return o
        return -1

    def bit(self, b: int, out: list):
        i = self.n
        self.sr = ((self.sr << 1) | (b & 1)) & M64
        self.n += 1
        if not self.synced:
            if self.n < 26:
                return
            w = self.sr & M26
            s = syndrome(w)
            if s not in OFFSET_WORDS:
                return
            o = OFFSET_WORDS.index(s)
            idx = OFFSET_BLOCK[o]
            if self.pending is not None:
                p, q = self.pending
                d = i - p
                if d % 26 == 0 and 1 <= d // 26 <= 4 and (q + d // 26) % 4 == idx:
                    self.acquired += 1
                    self.bad_run = 0
                    self._clear_assembly()
                    self.synced = 1
                    self.expect = idx
                    self.good += 1
                    self._place(w, o)
                    self._end_of_block(out)
                    self.judge_at = i + 27
                    self.pending = None
                    return
            self.pending = (i, idx)
            return
        if i != self.judge_at:
            return
        nominal = (self.sr >> 1) & M26
        early = (self.sr >> 2) & M26
        late = self.sr & M26
        o = self._match(nominal, self.expect)
        if o >= 0:
            self.good += 1
            self.bad_run = 0
            self._place(nominal, o)
            self.judge_at = i + 26
            self._end_of_block(out)
            return
        o = self._match(early, self.expect)
        if o >= 0:
            self.good += 1
            self.slips += 1
            self.bad_run = 0
            self._place(early, o)
            self.judge_at = i + 25
            self._end_of_block(out)
            return
        o = self._match(late, self.expect)
        if o >= 0:
            self.good += 1
            self.slips += 1
            self.bad_run = 0
            self._place(late, o)
            self.judge_at = i + 27
            self._end_of_block(out)
            return
        s = syndrome(nominal)
        for o in BLOCK_OFFSETS[self.expect]:
            e = self.tab[s ^ OFFSET_WORDS[o]]
            if e:
                self.corrected += 1
                self._place(nominal ^ e, o, corrected=True)
                self.judge_at = i + 26
                self._end_of_block(out)
                return
        self.bad += 1
        self.bad_run += 1
        self.judge_at = i + 26
        if self.bad_run == self.loss_blocks:
            self._lose()
            return
        self._end_of_block(out)

    def call(self, nbits: int, bits) -> list:
        """One call: the group records it emits, as tuples (w, ok, corrected, flags, reserved, bits).
        nbits outside -2 .. 256 consumes nothing, like -1."""
        out: list = []
        if nbits == NBITS_POISONED:
            if self.synced:
                self.synced = 0
                self.lost += 1
            self.pending = None
            self._clear_assembly()
            return out
        if nbits < 0 or nbits > MAX_BITS:
            return out
        for k in range(nbits):
            self.bit(int(bits[k]), out)
        assert len(out) <= MAX_GROUPS
        return out

    def stats(self) -> dict:
        d = {c: getattr(self, c) for c in COUNTERS}
        d["synced"] = self.synced
        return d

    def state(self) -> tuple:
        return (self.sr, self.n, self.synced, self.expect, self.judge_at if self.synced else 0, self.bad_run, self.pending,
                tuple(self.w), self.ok, self.cmask, self.flags) + tuple(getattr(self, c) for c in COUNTERS)


def records(groups) -> np.ndarray:
    """Group tuples as a GROUP_DTYPE array."""
    a = np.zeros(len(groups), GROUP_DTYPE)
    for k, g in enumerate(groups):
        a[k] = (g[0], g[1], g[2], g[3], g[4], g[5])
    return a


def decode(bits, max_burst: int = 2, loss_blocks: int = 8):
    """A whole stream through one channel: (group tuples, Channel)."""
    ch = Channel(max_burst, loss_blocks)
    out: list = []
    for b in bits:
        ch.bit(int(b), out)
    return out, ch


def group_line(ch: int, g) -> str:
    """The PREFIX.groups line of a group tuple."""
    f = []
    for b in range(4):
        if not (g[1] >> b) & 1:
            f.append("----")
        else:
            f.append("%04X%s" % (g[0][b], "*" if (g[2] >> b) & 1 else ""))
    return "ch %d bits %d %s" % (ch, g[5], " ".join(f))


# ------------------------------------------------------------------ text layer, for the tests
def station_ps(groups):
    """(the PIs seen with block A ok, the PS once all four segments of type-0 groups were seen or None)."""
    pis, ps, seen = set(), [" "] * 8, 0
    done = None
    for g in groups:
        w, ok = g[0], g[1]
        if ok & 1:
            pis.add(w[0])
        if (ok & 2) and (w[1] >> 12) == 0 and (ok & 8):
            seg = w[1] & 3
            c = [chr(w[3] >> 8), chr(w[3] & 0xFF)]
            if (seen >> seg) & 1 and ps[2 * seg: 2 * seg + 2] != c:
                seen = 0                      # a segment already seen changed: the name starts again
            ps[2 * seg: 2 * seg + 2] = c
            seen |= 1 << seg
            if seen == 15 and done is None:
                done = "".join(ps)
    return pis, done


def blocks_to_bits(blocks) -> list:
    """26-bit blocks to the bit list, first bit received first."""
    out = []
    for blk in blocks:
        out.extend((blk >> (25 - i)) & 1 for i in range(26))
    return out


# ------------------------------------------------------------------ test streams (no DSP)
def make_streams(synth, nbits: int = 3016, seed: int = 5):
    """Eight bit streams of about nbits bits, as lists of 0/1: a clean 0A cycle; 0A/2A/4A mixed; bits
    deleted and doubled every ~300 bits; bursts of length 1..5 in chosen blocks; a 14-bit phase jump;
    uniformly random bits; all zeros; a second clean cycle (for the channel that gets -1 and -2 calls)."""
    rs = np.random.Generator(np.random.PCG64(seed))
    ngroups = (nbits + 103) // 104

    def cycle(pi, ps):
        blocks = []
        for k in range(ngroups):
            blocks += synth.rds_group_0a(pi, 10, k & 3, ps, af=((225 + (k & 1)) << 8) | (10 + k % 7))
        return blocks

    def mixed(pi):
        text = "RadioText of the synthetic station, sixty-four characters long.."
        blocks = []
        for k in range(ngroups):
            if k % 3 == 0:
                blocks += synth.rds_group_0a(pi, 5, (k // 3) & 3, "MIXED 01")
            elif k % 3 == 1:
                blocks += synth.rds_group_2a(pi, 5, 0, (k // 3) & 15, text)
            else:
                blocks += synth.rds_group_4a(pi, 5, 58849 + k, k % 24, (7 * k) % 60, (k % 9) - 4)
        return blocks

    clean = blocks_to_bits(cycle(0x2001, "CLEAN 00"))
    s1 = blocks_to_bits(mixed(0x2002))
    s2 = blocks_to_bits(cycle(0x2003, "SLIPS 02"))
    out2, k = [], 0
    for i, b in enumerate(s2):                       # every 301 bits: delete, delete, double, double, ...
        if i and i % 301 == 0:
            k += 1
            if (k - 1) % 4 < 2:
                continue
            out2.append(b)
        out2.append(b)
    s3 = blocks_to_bits(cycle(0x2004, "BURST 03"))
    for blk in range(3, len(s3) // 26, 5):           # a burst of length 1..5 in every fifth block
        length = 1 + (blk // 5) % 5
        pos = 26 * blk + int(rs.integers(0, 27 - length))
        s3[pos] ^= 1
        s3[pos + length - 1] ^= 1
        for m in range(1, length - 1):
            s3[pos + m] ^= int(rs.integers(0, 2))
    s4 = blocks_to_bits(cycle(0x2005, "JUMP  04"))
    at = 26 * 4 * 12 + 7
    s4 = s4[:at] + [int(v) for v in rs.integers(0, 2, 14)] + s4[at:]
    s5 = [int(v) for v in rs.integers(0, 2, nbits)]
    s6 = [0] * nbits
    s7 = blocks_to_bits(cycle(0x2008, "POISON07"))
    return [clean, s1, out2, s3, s4, s5, s6, s7]
