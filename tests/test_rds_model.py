"""CPU: the RDS group decoder's definition (tests/rds_model.py) -- the correction table, the block code,
the fixtures' streams, call-split invariance -- and the library's host-only helpers against it. No GPU."""
from __future__ import annotations

import json

import numpy as np
import pytest

import rds_model as rm
from conftest import GOLD


# ---------------------------------------------------------------- correction table and syndrome
@pytest.mark.parametrize("max_burst,entries", [(5, 367), (2, 51), (0, 0)])
def test_correction_table_sizes(max_burst, entries):
    tab, n = rm.correction_table(max_burst)
    assert n == entries
    assert np.count_nonzero(tab) == entries and tab[0] == 0      # distinct, non-zero syndromes
    for s in np.nonzero(tab)[0]:
        assert rm.syndrome(int(tab[s])) == s


def test_library_helpers_equal_the_model(pkg):
    for mb in range(6):
        tab, n = pkg.rds_correction_table(mb)
        want, wn = rm.correction_table(mb)
        assert n == wn and np.array_equal(tab, want), mb
    rs = np.random.Generator(np.random.PCG64(1))
    for w in [int(v) for v in rs.integers(0, 1 << 26, 1000)] + list(range(1024)):
        assert pkg.rds_syndrome(w) == rm.syndrome(w), hex(w)
    assert pkg.lib().sdr_rds_correction_table(6, None, None) == -1
    assert pkg.lib().sdr_rds_correction_table(-1, None, None) == -1
    o = pkg.rds_opts()
    assert (o.max_burst, o.loss_blocks) == (2, 8) == (rm.DEFAULTS["max_burst"], rm.DEFAULTS["loss_blocks"])
    assert pkg.rds_group_dtype().itemsize == 16 == rm.GROUP_DTYPE.itemsize
    for name in rm.GROUP_DTYPE.names:
        assert rm.GROUP_DTYPE.fields[name][1] == getattr(pkg.RdsGroup, name).offset, name
    assert pkg.rds_stats_dtype().names == rm.COUNTERS + ("synced",)
    assert pkg.lib().sdr_version() == 3


def test_parity_rows_are_the_syndrome():
    rows = rm.parity_rows()
    rs = np.random.Generator(np.random.PCG64(2))
    for w in [int(v) for v in rs.integers(0, 1 << 26, 500)]:
        s = sum((bin(w & rows[r]).count("1") & 1) << r for r in range(10))
        assert s == rm.syndrome(w)


# ---------------------------------------------------------------- every rds_group_0a block
def _blocks(synth):
    out = []
    for ch in (0, 3, 77):
        for seg in range(4):
            out += list(enumerate(synth.rds_group_0a(0x1000 + ch, (ch * 7 + 10) % 32, seg, f"MI355X{ch:02d}")))
    return out


def test_blocks_match_their_own_offset_only(synth):
    own = {0: 0, 1: 1, 2: 2, 3: 4}
    for b, blk in _blocks(synth):
        s = rm.syndrome(blk)
        assert [o for o in range(5) if s == rm.OFFSET_WORDS[o]] == [own[b]], (b, hex(blk))


def test_every_burst_up_to_5_is_corrected_back(synth):
    tab5, _ = rm.correction_table(5)
    own = {0: 0, 1: 1, 2: 2, 3: 4}
    for b, blk in _blocks(synth)[:8]:
        for e in rm.burst_patterns(5):
            s = rm.syndrome(blk ^ e) ^ rm.OFFSET_WORDS[own[b]]
            assert int(tab5[s]) == e and (blk ^ e ^ int(tab5[s])) == blk


def test_a_3_bit_burst_is_not_corrected_at_max_burst_2(synth):
    tab2, _ = rm.correction_table(2)
    own = {0: 0, 1: 1, 2: 2, 3: 4}
    three = [e for e in rm.burst_patterns(3) if e not in set(rm.burst_patterns(2))]
    assert len(three) == 48
    for b, blk in _blocks(synth)[:8]:
        for e in three:
            fix = int(tab2[rm.syndrome(blk ^ e) ^ rm.OFFSET_WORDS[own[b]]])
            assert fix == 0 or (blk ^ e ^ fix) != blk        # never back to the original: e is not in the table


# ---------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("ch", [0, 3])
def test_model_on_the_long_fixture(golden_long, ch):
    rec = golden_long["channels"][str(ch)]
    bits = [int(x) for b in rec["blocks"] if b.get("bits") for x in b["bits"]]
    groups, st = rm.decode(bits)
    pis, ps = rm.station_ps(groups)
    assert pis == {0x1000 + ch}
    assert ps == f"MI355X{ch:02d}"
    full = sum(1 for g in groups if g[1] == 15)
    ref = rec["rds_text"].count("PI:")
    print(f"ch {ch}: {len(bits)} bits, {len(groups)} groups, {full} complete, reference PI lines {ref}, {st.stats()}")
    assert full >= ref
    assert full == {0: 62, 3: 57}[ch]                   # the counts the definition was designed on
    if ch == 0:
        assert st.slips >= 1


@pytest.mark.parametrize("ch", [0, 3])
def test_model_on_the_24_block_fixture(golden, ch):
    fixture = json.loads((GOLD / "rds_groups_mode0.json").read_text())["channels"][str(ch)]
    model = rm.Channel()
    groups = []
    for blk in golden[f"ch{ch}_bits"]:
        s = str(blk)
        groups += model.call(len(s) if s else -1, [int(x) for x in s])
    assert [rm.group_line(ch, g) for g in groups] == fixture["groups"]
    assert model.stats() == fixture["stats"]
    assert len(groups) == 6 and groups[0][1] == 12          # the first group is partial: C and D only
    assert rm.station_ps(groups) == ({0x1000 + ch}, f"MI355X{ch:02d}")
    if ch == 0:
        assert [g[5] for g in groups] == [96, 200, 304, 408, 512, 616]


# ---------------------------------------------------------------- call-split invariance
def _stream(synth):
    """3000 bits with slips, bursts and a phase jump."""
    s = rm.make_streams(synth, 3016)
    a, b, c = s[2][:1000], s[3][1000:2000], s[4][2000:]
    return (a + b + c)[:3000]


def _feed(stream, sizes, **opts):
    ch = rm.Channel(**opts)
    out, at = [], 0
    for n in sizes:
        if n < 0:
            out += ch.call(n, [])
            continue
        n = min(n, len(stream) - at)
        out += ch.call(n, stream[at:at + n])
        at += n
    assert at == len(stream)
    return out, ch.state()


def test_call_split_invariance(synth):
    stream = _stream(synth)
    want, ch = rm.decode(stream)
    assert ch.slips >= 2 and ch.bad >= 1 and ch.groups >= 20
    rs = np.random.Generator(np.random.PCG64(9))
    plans = {"one": [1] * 3000, "36/37": [36, 37] * 42, "256": [256] * 12,
             "random": [int(v) for v in rs.choice((0, -1, 1, 2, 25, 26, 27, 36, 37, 100, 255, 256), 400)] + [256] * 12}
    for name, sizes in plans.items():
        got, state = _feed(stream, sizes)
        assert got == want, name
        assert state == ch.state(), name


def test_a_poisoned_call_drops_sync(synth):
    stream = _stream(synth)
    ch = rm.Channel()
    ch.call(256, stream[:256])
    assert ch.synced and ch.lost == 0
    n = ch.n
    assert ch.call(rm.NBITS_POISONED, []) == []
    assert not ch.synced and ch.lost == 1 and ch.pending is None and ch.ok == 0 and ch.n == n
    assert ch.call(rm.NBITS_POISONED, []) == [] and ch.lost == 1        # no sync to drop: nothing counted
    ch.call(256, stream[256:512])
    assert ch.synced and ch.acquired == 2
    for bad in (dict(max_burst=6), dict(max_burst=-1), dict(loss_blocks=0), dict(loss_blocks=65)):
        with pytest.raises(ValueError):
            rm.Channel(**bad)


def test_why_the_default_burst_limit_is_2(golden_long):
    """On channel 3 of the long fixture max_burst = 5 miscorrects a block into a PS byte (0xAC); 2 does not."""
    bits = [int(x) for b in golden_long["channels"]["3"]["blocks"] if b.get("bits") for x in b["bits"]]
    odd = {}
    for mb in (2, 5):
        groups, _ = rm.decode(bits, mb)
        chars = set()
        for w, ok, *_ in groups:
            if ok & 2 and ok & 8 and (w[1] >> 12) == 0:
                chars |= {w[3] >> 8, w[3] & 0xFF}
        odd[mb] = sorted(c for c in chars if not 0x20 <= c <= 0x7E)
    assert odd == {2: [], 5: [0xAC]}
