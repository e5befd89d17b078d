"""CPU: the model of the RDS soft decisions (tests/rds_soft_model.py) against the models it extends, its own
rules on hand-built (bits, soft) cases, and the independence of the result from the cut into calls. No GPU."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import rds_model as rm
import rds_soft_model as sm
import rds_track_model as tm

BLOCK = sm.BLOCK             # the block the hand-built cases damage: group 2, block B


@pytest.fixture(scope="module")
def streams(synth):
    return rm.make_streams(synth)


@pytest.fixture(scope="module")
def soft_streams(synth):
    return sm.make_soft_streams(synth)


@pytest.fixture(scope="module")
def clean(streams):
    """(bits, groups): the clean stream and what the hard decoder makes of it; it starts on a group boundary, so
    block k is bits 26 k .. 26 k + 25, judged at i = 26 (k + 1) with the window raws 26 k - 1 .. 26 k + 25."""
    return streams[0], rm.decode(streams[0])[0]


SEVEN = sm.SEVEN
damaged = sm.damaged


def test_the_hand_built_positions_hide_no_code_word():
    """A pattern other than the errors matches when it and the errors together make a code word (the false
    acceptance of any Chase step); the cases below want none, so that what they see is the rule under test."""
    for k in range(1, 8):
        for sub in itertools.combinations(SEVEN, k):
            e = 0
            for p in sub:
                e ^= sm.toggle(p)
            assert rm.syndrome(e) != 0 and e != 0, sub
    assert [sm.toggle(p) for p in (0, 1, 25, 26)] == [1 << 25, 3 << 24, 3, 1]


def soft_flag(group, b: int) -> int:
    return (group[3] >> (sm.GROUP_SOFT_SHIFT + b)) & 1


# ------------------------------------------------------------------ the tracker
def _track_rows():
    rows = {"noise_rows": tm.noise_rows(3, 40000)[0], "off_grid": tm.off_grid(4, 40000),
            "walking_early": tm.walking(5, 40000, 16 * tm.B - 1, False), "walking_late": tm.walking(6, 40000, 16 * tm.B + 1, True),
            "wrong_half": tm.wrong_half(7, 40000)}
    return rows


@pytest.mark.parametrize("name", ["noise_rows", "off_grid", "walking_early", "walking_late", "wrong_half"])
def test_the_soft_tracker_is_the_tracker(name):
    x = _track_rows()[name]
    rs = np.random.Generator(np.random.PCG64(1))
    cuts = [0]
    while cuts[-1] < len(x):
        cuts.append(min(len(x), cuts[-1] + int(rs.choice((1, 77, 78, 79, 1000, 2836, 3073, 8000)))))
    rows = [x[a:b] for a, b in zip(cuts, cuts[1:])]
    old, new = tm.Channel(), sm.TrackChannel()
    softs = []
    for r in rows:
        nb0, b0 = old.call(r)
        nb1, b1, s1 = new.call(r)
        assert (nb0, b0) == (nb1, b1) and old.state() == new.state() and len(s1) == max(nb1, 0)
        softs += s1
    assert old.bits > 400 and max(softs) <= sm.SOFT_MAX
    # the soft values do not depend on the cut either
    whole_bits, whole_soft, _ = sm.track_soft([x[k:k + 2836] for k in range(0, len(x), 2836)])
    assert whole_soft == softs
    if name == "wrong_half":
        assert old.half_moves >= 1


def test_a_poisoned_call_gives_no_soft_values():
    x = tm.noise_rows(9, 6000)[0]
    ch, old = sm.TrackChannel(), tm.Channel()
    assert ch.call(x[:3000])[0] == old.call(x[:3000])[0]
    bad = x[3000:6000].copy()
    bad[17] = np.nan
    assert ch.call(bad) == (tm.NBITS_POISONED, [], []) and old.call(bad)[0] == tm.NBITS_POISONED
    assert ch.state() == old.state()
    assert ch.call(x[:0]) == (0, [], [])


def test_soft_is_the_on_time_correlator():
    amp = 300
    x = (tm.chips([1, 0] * 60, float(amp)) / np.float32(1 << tm.QSHIFT)).astype(np.float32)
    _, soft, ch = sm.track_soft([x])
    assert soft and set(soft) == {(tm.B * amp) >> 6}            # a clean bit: |c| = B * amp
    assert (tm.B * tm.QMAX) >> 6 == sm.SOFT_MAX == 39934 < 65536


# ------------------------------------------------------------------ the decoder: L = 0 and the cut
def test_soft_bits_0_is_the_hard_decoder(streams, soft_streams):
    for c, (s, v) in enumerate(zip(streams + soft_streams[0], sm.random_softs(streams) + soft_streams[1])):
        g0, ch0 = rm.decode(s)
        g1, ch1 = sm.decode(s, v, soft_bits=0)
        assert g0 == g1 and ch1.state()[:len(ch0.state())] == ch0.state(), c
        assert ch1.soft_stats() == dict(soft_blocks=0, soft_flips=0, soft_bits=0, reserved=0)
        assert all(g[3] >> sm.GROUP_SOFT_SHIFT == 0 and g[4] == 0 for g in g1)


def _cut_run(bits, soft, sizes, L, poison_at=(), idle_every=0):
    """One channel fed in calls of the sizes drawn from `sizes` (cycled); a -2 call in front of the stream
    positions `poison_at`, a -1 and an out-of-range call every idle_every calls."""
    ch = sm.Channel(soft_bits=L)
    out, at, k = [], 0, 0
    poison = sorted(poison_at)
    sizes = itertools.cycle(sizes)
    while at < len(bits):
        n = min(next(sizes), len(bits) - at)
        if poison and at + n > poison[0]:
            n = poison[0] - at
            if n == 0:
                poison.pop(0)
                out += ch.call(rm.NBITS_POISONED, [], [])
                continue
        k += 1
        if idle_every and k % idle_every == 0:
            before = ch.state()
            assert ch.call(-1, bits[at:], soft[at:]) == [] and ch.call(257, bits[at:], soft[at:]) == [] and ch.state() == before
        out += ch.call(n, bits[at:at + n], soft[at:at + n])
        at += n
    return out, ch


@pytest.mark.parametrize("L", [1, 4, 6])
def test_the_cut_does_not_matter(soft_streams, L):
    rs = np.random.Generator(np.random.PCG64(L))
    for c, (s, v) in enumerate(zip(*soft_streams)):
        s, v = s[:1600], v[:1600]
        want, ch = sm.decode(s, v, soft_bits=L)
        for sizes in ([1], [36, 37], [256], [int(x) for x in rs.integers(0, 257, 50)]):
            got, g = _cut_run(s, v, sizes, L, idle_every=3)
            assert got == want and g.state() == ch.state(), (c, sizes[:3])
        # with poisoned calls at the same places of the stream, again whatever the cut
        ref, r = _cut_run(s, v, [256], L, poison_at=(700, 701, 1300))
        for sizes in ([1], [36, 37], [int(x) for x in rs.integers(0, 257, 50)]):
            got, g = _cut_run(s, v, sizes, L, poison_at=(700, 701, 1300), idle_every=5)
            assert got == ref and g.state() == r.state(), (c, sizes[:3])
        if c == 0:
            assert ch.soft_blocks >= 3 and r.lost >= 2            # the step runs, and the poisoned calls drop sync


def test_the_soft_streams_do_what_they_were_built_for(soft_streams):
    pops = set()
    for c, (s, v) in enumerate(zip(*soft_streams)):
        hard = rm.decode(s)[1]
        ch = sm.Channel(soft_bits=6)
        out = []
        for b, q in zip(s, v):
            before = ch.soft_blocks
            ch.bit(b, q, out)
            if ch.soft_blocks != before:
                pops.add(bin(ch.last_win[1]).count("1"))
        if c in (0, 1, 3, 7):
            assert ch.soft_blocks >= 20 and ch.bad >= 3 and ch.bad < hard.bad, (c, ch.stats(), hard.stats())
    assert pops == {1, 2, 3, 4, 5, 6}


# ------------------------------------------------------------------ the decoder: hand-built cases
@pytest.mark.parametrize("p", range(27))
def test_one_raw_error_anywhere_in_the_window(clean, p):
    bits, groups = clean
    b, v = damaged(bits, {p: 5})
    got, ch = sm.decode(b, v, max_burst=0, soft_bits=6)
    assert [g[0] for g in got] == [g[0] for g in groups] and ch.bad == 0
    g = got[BLOCK // 4]
    assert soft_flag(g, BLOCK % 4) and (g[2] >> (BLOCK % 4)) & 1 and g[4] == 0
    # an edge raw also stands behind the neighbouring block's last / first diff bit: that block takes the step too
    assert ch.soft_blocks == (2 if p in (0, 26) else 1) == ch.corrected and ch.soft_flips == ch.soft_blocks
    assert ch.last_win[1] == 1 and bin(ch.last_win[2]).count("1") == (1 if p in (0, 26) else 2)
    hard = rm.decode(b, max_burst=0)[1]
    assert hard.bad == ch.soft_blocks and hard.corrected == 0


def test_six_errors_on_the_six_least_reliable(clean):
    bits, groups = clean
    flips = {p: j + 1 for j, p in enumerate(SEVEN[:6])}
    b, v = damaged(bits, flips)
    got, ch = sm.decode(b, v, soft_bits=6)
    assert [g[0] for g in got] == [g[0] for g in groups] and ch.bad == 0
    assert ch.soft_blocks == 1 and ch.soft_flips == 6 and ch.last_win[:2] == (21, 63)
    assert rm.decode(b)[1].bad == 1


def test_seven_errors_are_not_corrected(clean):
    bits, groups = clean
    flips = {p: j + 1 for j, p in enumerate(SEVEN)}
    b, v = damaged(bits, flips)
    got, ch = sm.decode(b, v, max_burst=0, soft_bits=6)
    assert ch.soft_blocks == 0 and ch.bad == 1 and not (got[BLOCK // 4][1] >> (BLOCK % 4)) & 1


def test_the_seventh_least_reliable_is_out_of_reach(clean):
    bits, groups = clean
    quiet = {2: (1, False), 1: (2, False), 6: (3, False), 11: (4, False), 8: (5, False), 17: (6, False)}
    b, v = damaged(bits, {**quiet, 13: 7})
    got, ch = sm.decode(b, v, max_burst=0, soft_bits=6)
    assert ch.soft_blocks == 0 and ch.bad == 1
    b, v = damaged(bits, {**quiet, 13: 6})                     # a tie with position 17: the older one is the candidate
    got, ch = sm.decode(b, v, max_burst=0, soft_bits=6)
    assert ch.soft_blocks == 1 and ch.bad == 0 and ch.last_win[1] == 32


def test_every_soft_bits_reaches_its_own_depth(clean):
    bits, _ = clean
    order = SEVEN[:6]
    for k in range(1, 7):
        b, v = damaged(bits, {p: j + 1 for j, p in enumerate(order[:k])})
        for L in range(0, 7):
            ch = sm.decode(b, v, max_burst=0, soft_bits=L)[1]
            assert (ch.soft_blocks, ch.bad) == ((1, 0) if k <= L else (0, 1)), (k, L)
            if k <= L:
                assert ch.last_win[1] == (1 << k) - 1 and ch.soft_flips == k
    for L in (-1, 7):
        with pytest.raises(ValueError):
            sm.Channel(soft_bits=L)


@pytest.mark.parametrize("level", [0, 1000, 65535])
def test_equal_softs_make_the_six_oldest_the_candidates(clean, level):
    bits, groups = clean
    b, v = damaged(bits, {p: level for p in range(1, 6)}, others=level)
    got, ch = sm.decode(b, v, max_burst=0, soft_bits=6)
    assert ch.soft_blocks == 1 and ch.bad == 0 and ch.last_win[:2] == (5 * level, 0b111110)
    assert [g[0] for g in got] == [g[0] for g in groups]
    b, v = damaged(bits, {6: level}, others=level)
    ch = sm.decode(b, v, max_burst=0, soft_bits=6)[1]
    assert ch.soft_blocks == 0 and ch.bad == 1


_toggle_sets = sm.toggle_sets


def test_two_matching_patterns_on_block_c(clean):
    """Block C takes offset C and C': with D a set of four raws whose toggles turn a C word into a C' word,
    errors on two of them leave two patterns that match, the two that undo the errors (C) and the other two (C')."""
    bits, groups = clean
    block = 4 * 2 + 2
    D, e = next(_toggle_sets(rm.OFFSET_WORDS[2] ^ rm.OFFSET_WORDS[3]))
    word = 0
    for k in range(26):
        word = (word << 1) | bits[26 * block + k]

    def run(softs):                                             # errors on D[0], D[1]; the softs of D in order
        flips = {D[0]: softs[0], D[1]: softs[1], D[2]: (softs[2], False), D[3]: (softs[3], False)}
        b, v = damaged(bits, flips, block=block)
        got, ch = sm.decode(b, v, max_burst=0, soft_bits=4)
        assert ch.soft_blocks == 1 and ch.bad == 0
        return got[block // 4], ch

    g, ch = run((1, 2, 3, 4))                                   # the errors are the lighter pair: C, the clean word
    assert g[0] == groups[block // 4][0] and not g[3] & 1 and ch.last_win[:2] == (3, 0b0011)
    g, ch = run((3, 4, 1, 2))                                   # the other pair is lighter: the C' word wins
    assert g[0][2] == ((word ^ e) >> 10) & 0xFFFF and g[3] & 1 and ch.last_win[:2] == (3, 0b0011)
    g, ch = run((2, 3, 1, 4))                                   # equal weights 5 = 5: the lower m wins
    order = sorted(range(4), key=lambda j: ((2, 3, 1, 4)[j], D[j]))      # candidate j is D[order[j]]
    m_errors = sum(1 << j for j in range(4) if order[j] in (0, 1))
    m_other = 15 ^ m_errors
    assert ch.last_win[:2] == (5, min(m_errors, m_other))
    assert (g[0] == groups[block // 4][0]) == (m_errors < m_other)


def test_soft_wins_over_the_burst_table(clean):
    """One raw error is a burst of two diff bits, which the table corrects; when the raw is no candidate and
    three candidates together with it make a code word, the soft step places another word first."""
    bits, groups = clean
    D, e = next(_toggle_sets(0))
    word = 0
    for k in range(26):
        word = (word << 1) | bits[26 * BLOCK + k]
    b, v = damaged(bits, {D[0]: 900, D[1]: (1, False), D[2]: (2, False), D[3]: (3, False)})
    hard, hch = rm.decode(b)
    assert hard == rm.decode(b, max_burst=2)[0] and hch.corrected == 1 and [g[0] for g in hard] == [g[0] for g in groups]
    got, ch = sm.decode(b, v, soft_bits=3)
    g = got[BLOCK // 4]
    assert ch.soft_blocks == 1 and ch.corrected == 1 and ch.last_win[1] == 7 and soft_flag(g, BLOCK % 4)
    assert g[0][BLOCK % 4] == ((word ^ e) >> 10) & 0xFFFF != groups[BLOCK // 4][0][BLOCK % 4]
    got, ch = sm.decode(b, v, soft_bits=2)                      # out of reach: the burst table as before
    assert got == hard and ch.soft_blocks == 0


def test_a_window_wholly_in_the_history(clean):
    bits, _ = clean
    b, v = damaged(bits, {0: 1, 9: 2, 26: 3})
    whole, ch = sm.decode(b, v, soft_bits=6)
    one = sm.Channel(soft_bits=6)
    got = []
    for k in range(len(b)):
        got += one.call(1, b[k:k + 1], v[k:k + 1])             # every judgement's window is the history alone
    assert got == whole and one.state() == ch.state() and ch.soft_blocks >= 1
    assert len(one.hist) == sm.HIST >= 28


def test_no_judgement_before_its_window_is_in(streams, soft_streams):
    """The first judgement after a reset is at bit FIRST_JUDGEMENT = 78 or later (bit() asserts it), so no window
    reaches in front of the stream; the earliest possible one is reached by a stream that starts on a block."""
    first = []

    class Spy(sm.Channel):
        def bit(self, b, soft, out):
            if self.synced and self.n == self.judge_at:
                first.append(self.n)
            super().bit(b, soft, out)

    for s, v in zip(streams + soft_streams[0], sm.random_softs(streams) + soft_streams[1]):
        del first[:]
        ch = Spy(soft_bits=6)
        out = []
        for b, q in zip(s, v):
            ch.bit(b, q, out)
        assert not first or min(first) >= sm.FIRST_JUDGEMENT
    ch = Spy(soft_bits=6)
    del first[:]
    for b in streams[0][:200]:
        ch.bit(b, 7, [])
    assert first[0] == sm.FIRST_JUDGEMENT == 78


def test_group_line_marks_soft_blocks(clean):
    bits, _ = clean
    b, v = damaged(bits, {5: 1})
    b2 = list(b)
    b2[26 * 14 + 3] ^= 1                                        # a single diff bit: the burst table's
    v2 = list(v)
    v2[26 * 14 + 2] = v2[26 * 14 + 3] = 65535
    got, ch = sm.decode(b2, v2, soft_bits=1)
    lines = [sm.group_line(3, g) for g in got]
    assert ch.soft_blocks == 1 and ch.corrected == 2
    assert lines[BLOCK // 4].split()[4 + BLOCK % 4].endswith("~") and lines[3].split()[4 + 2].endswith("*")
    assert [sm.group_line(3, g) for g in rm.decode(bits)[0]] == [rm.group_line(3, g) for g in rm.decode(bits)[0]]
