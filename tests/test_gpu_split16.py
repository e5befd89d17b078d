"""GPU: the 16-bit wideband splitter (include/sdr_amd.h: sdr_split16_*, the kernel k_split16 of sdr_split16.hip)
against the integer model of tests/split16_model.py. The definition is all integer, so every comparison is byte
for byte and every clip counter and peak is compared exactly; there is no tolerance anywhere."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import scan_model as sm
import split16_model as s16
import split_model as spm
import tuner_model as tm

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
# (mode, W, nwide, nblocks): the s8 suite's shapes (tests/test_gpu_split.py): every W, the history across blocks
# and the zero history of block 0, both batch positions, a whole and a ragged number of workgroups and tiles
SHAPES = [(3, 4, 2, 3), (1, 8, 1, 2), (0, 10, 2, 2)]
IDS = dict(ids=lambda s: "mode%d-W%d-n%d-b%d" % s)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_RANDOM: dict = {}


def _random(shape):
    """(wide int16 [nblocks][nwide][2 W block_iq], the model's flipped sums): full-range random samples with both
    ends of the range and the low bytes 0x00, 0x7F, 0x80, 0xFF certainly among them, made once, left unchanged."""
    if shape not in _RANDOM:
        mode, W, nwide, nblocks = shape
        n = 2 * W * spm.GEOM[mode][1]
        wide = np.random.default_rng(16000 + 10 * mode + W).integers(-32768, 32768, (nblocks, nwide, n), dtype=np.int16)
        for i, v in enumerate((-32768, 32767, 0x1200, 0x127F, -0x0D80, 0x12FF, -256, -129, -128, -1)):
            wide[:, :, 5 + i::997] = v
        _RANDOM[shape] = (wide, s16.sums(mode, W, wide))
    return _RANDOM[shape]


def _gpu(pkg, torch, mode, W, wide, shifts=None, pad_in=32, pad_out=32, sp=None, tables=None):
    """(rows u8 [nblocks][nwide R][2 block_iq], clips, peaks [nwide][R]) of a fresh splitter (or sp) over the
    blocks; shifts: one table for the run, tables: one per block, set before it. Input rows lie 2 W block_iq +
    pad_in values apart, output rows 2 block_iq + pad_out bytes; the output padding must come back untouched."""
    nblocks, nwide, n = wide.shape
    own = sp is None
    if own:
        sp = pkg.Splitter16(W, nwide, mode=mode)
    if shifts is not None:
        sp.set_shifts(shifts)
    nb = 2 * sp.block_iq
    out = []
    for b in range(nblocks):
        if tables is not None:
            sp.set_shifts(tables[b])
        hw = np.zeros((nwide, n + pad_in), np.int16)
        hw[:, :n] = wide[b]
        d = torch.from_numpy(hw).cuda()[:, :n]
        buf = torch.full((nwide * sp.rows, nb + pad_out), SENTINEL, dtype=torch.uint8, device="cuda")
        got = sp.block(d, out=buf[:, :nb])
        assert got.data_ptr() == buf.data_ptr()
        h = buf.cpu().numpy()
        assert np.all(h[:, nb:] == SENTINEL), f"block {b}: bytes past a row's end were written"
        out.append(h[:, :nb].copy())
    clips, peaks = sp.clips(), sp.peaks()
    if own:
        sp.close()
    return np.stack(out), clips, peaks


def _same(got, ref, what):
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at (block, row, byte) {bad[0].tolist()}: "
                             f"got {got[tuple(bad[0])]}, model {ref[tuple(bad[0])]}")


def _all_same(got, ref, what):
    _same(got[0], ref[0], what)
    assert np.array_equal(got[1], ref[1]), f"{what}: clips"
    assert np.array_equal(got[2], ref[2]), f"{what}: peaks"


@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_random_full_range(pkg, torch_cuda, shape):
    mode, W, nwide, nblocks = shape
    wide, acc = _random(shape)
    assert wide.min() == -32768 and wide.max() == 32767
    low = wide.view(np.uint16) & 0xFF
    assert all((low == v).any() for v in (0x00, 0x7F, 0x80, 0xFF))
    ref = s16.finish_all(acc, s16.SHIFT_DEFAULT[W])
    assert ref[2].max() < 2 ** 33
    _all_same(_gpu(pkg, torch_cuda, mode, W, wide), ref, f"shape {shape}")


def _mixed_table(W, nwide):
    """A shift per row that differs between neighbouring rows and between the streams, 1 and 33 among them."""
    R = 2 * W - 1
    base = s16.SHIFT_DEFAULT[W]
    t = np.array([[base - 6 + ((5 * r + 3 * w) % 9) for r in range(R)] for w in range(nwide)], np.int64)
    t[0, 0], t[-1, R - 1], t[0, R // 2] = 1, 33, 33 if nwide > 1 else base - 7
    return t


@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_mixed_shift_table(pkg, torch_cuda, shape):
    mode, W, nwide, nblocks = shape
    wide, acc = _random(shape)
    tab = _mixed_table(W, nwide)
    assert 1 in tab and 33 in tab and len(set(tab.ravel().tolist())) > 4
    assert (np.diff(tab, axis=1) != 0).all() and (nwide == 1 or (tab[0] != tab[1]).all())
    ref = s16.finish_all(acc, tab)
    s2 = np.repeat(tab, 2, axis=1)[None, :, None, :]
    v = 128 + ((acc + (np.int64(1) << (s2 - 1))) >> s2)
    assert (v < 0).any() and (v > 255).any() and (ref[0] == 0).any() and (ref[0] == 255).any()   # clips both ways
    assert ref[1].max() > 0 and (ref[1] == 0).any()
    got = _gpu(pkg, torch_cuda, mode, W, wide, shifts=tab)
    _all_same(got, ref, f"shape {shape}, mixed table")


_EXTREMES: dict = {}


def _extremes():
    """mode 3, W = 4, two blocks of eleven streams: all -32768, all +32767, all -1 (0xFFFF), values 0..255 only
    (high byte 0), multiples of 256 only (low byte 0), and for rows 0, W - 1 and 2 W - 2 a stream of zeros with
    windows that carry the signs of that row's acc_re tap column at full scale (32767 for positive, -32768 for
    negative: |acc| is as large as it gets), one in the middle of block 0 and one straddling the boundary between
    blocks 0 and 1; then the same three with the signs reversed (the largest negative sums)."""
    if not _EXTREMES:
        mode, W = 3, 4
        T, b = 16 * W, spm.GEOM[mode][1]
        M = spm.tap_matrix(W)
        rng = np.random.default_rng(77)
        s = np.zeros((11, 2 * 2 * W * b), np.int16)
        s[0], s[1], s[2] = -32768, 32767, -1
        s[3] = rng.integers(0, 256, s.shape[1])
        s[4] = rng.integers(-128, 128, s.shape[1]) * 256
        for i, r in enumerate((0, W - 1, 2 * W - 2)):
            pat = np.where(M[:, 2 * r] < 0, -32768, 32767).astype(np.int16)
            for t in (b // 2 + 3, b + 5):                           # W (b + 5) - T + 1 < W b: straddles
                s[5 + i, 2 * (W * t - T + 1):2 * (W * t + 1)] = pat
                s[8 + i, 2 * (W * t - T + 1):2 * (W * t + 1)] = -1 - pat
        wide = np.ascontiguousarray(s.reshape(11, 2, 2 * W * b).transpose(1, 0, 2))
        _EXTREMES["v"] = (mode, W, wide, s16.sums(mode, W, wide))
    return _EXTREMES["v"]


@pytest.mark.parametrize("shift", [33, 1])
def test_extremes(pkg, torch_cuda, shift):
    mode, W, wide, acc = _extremes()
    M = spm.tap_matrix(W)
    for i, r in enumerate((0, W - 1, 2 * W - 2)):                   # the windows do reach the largest |acc|
        top = 32767 * np.abs(M[:, 2 * r]).sum()
        assert np.abs(acc[:, 5 + i, :, 2 * r]).max() >= top
        assert np.abs(acc[:, 8 + i, :, 2 * r]).max() >= top
    assert acc.max() > 2 ** 31 and acc.min() < -2 ** 31 and np.abs(acc).max() <= s16.bounds(W)[1]
    ref = s16.finish_all(acc, shift)
    got = _gpu(pkg, torch_cuda, mode, W, wide, shifts=np.full((11, 2 * W - 1), shift))
    _all_same(got, ref, f"extremes shift {shift}")
    assert (ref[1].sum() > 0) == (shift == 1)


def test_identities_with_the_s8_splitter(pkg, torch_cuda):
    """An s8 capture widened as 256 x at shift s + 8, and sign-extended at shift s, gives the bytes and clip counts
    of Splitter at shift s on the same device."""
    torch = torch_cuda
    mode, W, nwide, nblocks = SHAPES[0]
    n = 2 * W * spm.GEOM[mode][1]
    wide8 = np.random.default_rng(7000 + 10 * mode + W).integers(-128, 128, (nblocks, nwide, n), dtype=np.int8)
    wide8[:, :, 5::997] = -128
    for s in (spm.SHIFT_DEFAULT[W], spm.SHIFT_DEFAULT[W] - 4, 24, 1):
        sp8 = pkg.Splitter(W, nwide, mode=mode, shift=s)
        ref = np.stack([sp8.block(torch.from_numpy(wide8[b]).cuda()).cpu().numpy() for b in range(nblocks)])
        ref_clips = sp8.clips()
        sp8.close()
        assert s > 1 or ref_clips.min() > 0                         # the clip counters are really compared
        full = np.full((nwide, 2 * W - 1), s)
        rows, clips, peaks = _gpu(pkg, torch, mode, W, s16.widen256(wide8), shifts=full + 8)
        _same(rows, ref, f"256 x at shift {s} + 8")
        assert np.array_equal(clips, ref_clips)
        rows, clips, peaks1 = _gpu(pkg, torch, mode, W, s16.sign_extend(wide8), shifts=full)
        _same(rows, ref, f"sign-extended at shift {s}")
        assert np.array_equal(clips, ref_clips) and np.array_equal(peaks, 256 * peaks1)


def test_determinism_and_layout(pkg, torch_cuda):
    shape = SHAPES[0]
    mode, W, nwide, nblocks = shape
    wide, acc = _random(shape)
    R = 2 * W - 1
    tab = _mixed_table(W, nwide)
    both = _gpu(pkg, torch_cuda, mode, W, wide, shifts=tab)
    again = _gpu(pkg, torch_cuda, mode, W, wide, shifts=tab)
    _all_same(again, both, "the same run twice")
    rows, clips, peaks = both
    sw = _gpu(pkg, torch_cuda, mode, W, np.ascontiguousarray(wide[:, ::-1]), shifts=tab[::-1])
    assert np.array_equal(sw[0][:, :R], rows[:, R:]) and np.array_equal(sw[0][:, R:], rows[:, :R])
    assert np.array_equal(sw[1][::-1], clips) and np.array_equal(sw[2][::-1], peaks)
    for w in range(nwide):
        alone = _gpu(pkg, torch_cuda, mode, W, np.ascontiguousarray(wide[:, w:w + 1]), shifts=tab[w:w + 1])
        assert np.array_equal(alone[0], rows[:, w * R:(w + 1) * R])
        assert np.array_equal(alone[1][0], clips[w]) and np.array_equal(alone[2][0], peaks[w])
    # unpadded, 16-byte aligned rows give the same bytes as the padded ones
    _all_same(_gpu(pkg, torch_cuda, mode, W, wide, shifts=tab, pad_in=0, pad_out=0), both, "unpadded")
    # input rows that are only 4-byte aligned, output rows that are only 2-byte aligned (the C ABI asks no more)
    _all_same(_gpu(pkg, torch_cuda, mode, W, wide, shifts=tab, pad_in=2, pad_out=6), both, "2-byte aligned rows")


def test_set_shifts_on_a_stream_peaks_and_reset(pkg, torch_cuda):
    """set_shifts before blocks 1 and 2 of three, all queued on one side stream with no host sync in between;
    then the clearing read of the peaks, and a reset that keeps the shifts and zeroes the rest."""
    torch = torch_cuda
    shape = SHAPES[0]
    mode, W, nwide, nblocks = shape
    wide, acc = _random(shape)
    R = 2 * W - 1
    base = np.full((nwide, R), s16.SHIFT_DEFAULT[W], np.int64)
    tables = np.stack([base, _mixed_table(W, nwide), base - 5])
    ref = s16.finish_all(acc, tables)
    assert ref[1].max() > 0
    sp = pkg.Splitter16(W, nwide, mode=mode)
    assert np.array_equal(sp.shifts, base)
    d = torch.from_numpy(wide).cuda()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    rows = []
    for b in range(nblocks):
        if b:
            t = tables[b].astype(np.int32)
            sp.set_shifts(t, stream=st)
            t[:] = 7                                                # the caller's table may go at once
        rows.append(sp.block(d[b], stream=st))
    st.synchronize()
    assert np.array_equal(sp.shifts, tables[2])
    _same(np.stack([r.cpu().numpy() for r in rows]), ref[0], "a table per block")
    assert np.array_equal(sp.clips(stream=st), ref[1])
    assert np.array_equal(sp.peaks(clear=True, stream=st), ref[2])
    assert not sp.peaks().any() and np.array_equal(sp.clips(), ref[1])      # the clearing read clears the peaks only
    # a refused table changes nothing
    for bad in (0, 34, -1):
        t = tables[2].copy()
        t[-1, -1] = bad
        with pytest.raises(pkg.SdrError):
            sp.set_shifts(t)
    with pytest.raises(pkg.SdrError):
        sp.set_shifts(tables[2][:, :-1])
    assert np.array_equal(sp.shifts, tables[2])
    sp.reset()
    assert not sp.clips().any() and not sp.peaks().any()
    got = _gpu(pkg, torch, mode, W, wide, sp=sp)                    # the shifts are still block 2's; history is zero
    sp.close()
    _all_same(got, s16.finish_all(acc, tables[2]), "after the reset")


def test_refused_calls_enqueue_nothing(pkg, torch_cuda):
    torch = torch_cuda
    shape = SHAPES[0]
    mode, W, nwide, nblocks = shape
    wide, acc = _random(shape)
    tab = _mixed_table(W, nwide)
    ref = s16.finish_all(acc, tab)
    sp = pkg.Splitter16(W, nwide, mode=mode)
    sp.set_shifts(tab)
    _gpu(pkg, torch, mode, W, wide[:2], sp=sp)                      # history, counters and peaks now non-zero
    sp.reset()
    # a refused call enqueues nothing: neither the rows, nor the history, nor the counters, nor the shifts move
    n, nb = 2 * wide.shape[2], 2 * sp.block_iq                      # bytes
    d = torch.from_numpy(wide[1]).cuda()
    buf = torch.full((nwide * sp.rows, nb), SENTINEL, dtype=torch.uint8, device="cuda")
    L, E = pkg.lib(), -1
    st = None
    assert L.sdr_split16_block(sp._h, d.data_ptr(), n - 4, buf.data_ptr(), nb, st) == E       # short wide stride
    assert L.sdr_split16_block(sp._h, d.data_ptr(), n + 2, buf.data_ptr(), nb, st) == E       # no multiple of 4
    assert L.sdr_split16_block(sp._h, d.data_ptr() + 2, n, buf.data_ptr(), nb, st) == E       # wide misaligned
    assert L.sdr_split16_block(sp._h, d.data_ptr(), n, buf.data_ptr(), nb - 2, st) == E       # short row stride
    assert L.sdr_split16_block(sp._h, d.data_ptr(), n, buf.data_ptr(), nb + 1, st) == E       # odd row stride
    assert L.sdr_split16_block(sp._h, d.data_ptr(), n, buf.data_ptr() + 1, nb + 2, st) == E   # odd rows address
    assert L.sdr_split16_block(sp._h, None, n, buf.data_ptr(), nb, st) == E
    assert L.sdr_split16_block(sp._h, d.data_ptr(), n, None, nb, st) == E
    assert L.sdr_split16_clips(sp._h, None, st) == E
    assert L.sdr_split16_peaks(sp._h, None, 0, st) == E
    assert L.sdr_split16_set_shifts(sp._h, None, st) == E
    bad = np.ascontiguousarray(tab, np.int32)
    bad[0, 1] = 34
    assert L.sdr_split16_set_shifts(sp._h, bad.ctypes.data_as(C.c_void_p), st) == E           # a bad shifts table
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    assert not sp.clips().any() and not sp.peaks().any()
    got = _gpu(pkg, torch, mode, W, wide, sp=sp)
    sp.close()
    _all_same(got, ref, "after reset and refused calls")
    h = C.c_void_p()
    for args in ((4, 4, 1, 0), (0, 5, 1, 0), (0, 4, 0, 0), (0, 4, 1, 34)):
        assert L.sdr_split16_create(C.byref(h), 0, *args) == E and not h.value


# The composite: a strong station (a float FM tone, split16_model.wide_composite16) at +200 kHz of the wide
# capture's centre and 0.45 of full scale -- the default shifts have a DC gain of 2, so this is what fills the
# output range without clipping -- and an FMMultiplexSource station at -7500 kHz, 63.5 dB below it. The weak
# amplitude was chosen on the CPU with the model chain below (rows -> scan_model picks): with the gain rule's
# shifts off block 0's peaks the int16 capture yields the weak station at 1e-3 and at 3e-4 and no longer at 1e-4;
# the same composite quantised to int8, at the s8 default shift, yields it at none of the three.
STRONG_KHZ, STRONG_AMP = 200, 0.45
WEAK_KHZ, WEAK_AMP = -7500, 3e-4
STRONG, WEAK = (7, 200), (1, -300)                                  # (row, kHz off the row's centre)


def test_composition_weak_station(pkg, oracle, synth, torch_cuda):
    """Mode 0, W = 8, 2 blocks, one stream. Asserted on the model first: the int16 capture, split with the shifts
    the rule gives block 0's peaks, yields both stations and nothing else; the int8 capture at the s8 default
    shift yields the strong one only. Then the GPU: peaks, shifts, rows and clips equal the model's, the Scanner's
    picks on them are the model's, and the tuner's fm_demod on the two stations' rows is the model's bit for bit."""
    torch = torch_cuda
    mode, W, nblocks = 0, 8, 2
    R = 2 * W - 1
    w16, w8, clipped = s16.wide_composite16(synth, W, nblocks, (WEAK_KHZ,), (WEAK_AMP,), tone=(STRONG_KHZ, STRONG_AMP))
    assert clipped == 0
    acc = s16.sums(mode, W, w16[:, None, :])
    peaks0 = s16.finish_all(acc[:1], s16.SHIFT_DEFAULT[W])[2]
    shifts = s16.shifts_for(peaks0, 90, W)
    assert shifts[0, WEAK[0]] <= s16.SHIFT_DEFAULT[W] - 3 and shifts[0, STRONG[0]] > s16.SHIFT_DEFAULT[W]
    ref, ref_clips, ref_peaks = s16.finish_all(acc, shifts)
    assert not ref_clips.any()
    ref8, ref8_clips = spm.run(mode, W, w8[:, None, :])
    assert not ref8_clips.any()

    def model_picks(rows):
        A, _tol, S = sm.rows_power(pkg, mode, [rows[b] for b in range(nblocks)])
        return spm.wide_pick(mode, W, (A / S).astype(np.float32), sm.pick), S

    picks16, S = model_picks(ref)
    picks8, _ = model_picks(ref8)
    assert picks16 == [WEAK, STRONG] and picks8 == [STRONG]         # the difference, on the model
    # the GPU, as the engine does it: block 0 into rows nobody reads, its peaks, the rule, set_shifts, reset
    sp, sc = pkg.Splitter16(W, 1, mode=mode), pkg.Scanner(mode, R)
    d = torch.from_numpy(w16[:, None, :]).cuda()
    sp.block(d[0])
    assert np.array_equal(sp.peaks(), peaks0)
    got_shifts = np.array([[pkg.split16_shift_for(int(p), 90, W=W) for p in peaks0[0]]])
    assert np.array_equal(got_shifts, shifts)
    sp.set_shifts(got_shifts)
    sp.reset()
    rows = [sp.block(d[b]) for b in range(nblocks)]
    for r in rows:
        sc.block(r)
    psd, seg = sc.psd()
    assert seg == S
    _same(np.stack([r.cpu().numpy() for r in rows]), ref, "composite")
    assert not sp.clips().any() and np.array_equal(sp.peaks(), ref_peaks)

    def lib_pick(row, **o):
        return pkg.scan_pick(mode, row, **o)

    assert spm.wide_pick(mode, W, psd, lib_pick) == picks16
    # the s8 splitter on the int8 capture: the strong station alone, on the GPU too
    sp8, sc8 = pkg.Splitter(W, 1, mode=mode), pkg.Scanner(mode, R)
    d8 = torch.from_numpy(w8[:, None, :]).cuda()
    for b in range(nblocks):
        sc8.block(sp8.block(d8[b]))
    assert spm.wide_pick(mode, W, sc8.psd()[0], lib_pick) == picks8
    # rows 1 and 7 lie 6 apart: a strided view of the split rows is the tuner's capture batch as it stands
    khz = [WEAK[1], STRONG[1]]
    pipe = pkg.Pipeline(2, mode=mode, rds_on=True, device=0)
    pipe.set_tuning([0, 1], khz, 2)
    want = tm.run_tuned(pkg, oracle, mode, ref[:, 1:8:6], [0, 1], khz)
    for b in range(nblocks):
        pipe.frontend_tuned(rows[b][1:8:6])
        fm = pipe.fm_demod().cpu().numpy()
        for c in range(2):
            assert np.array_equal(fm[c].view(np.uint32), want[c]["fm"][b].view(np.uint32)), f"fm_demod block {b} ch {c}"
    for h in (pipe, sc, sp, sc8, sp8):
        h.close()
