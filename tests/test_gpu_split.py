"""GPU: the wideband splitter (include/sdr_amd.h: sdr_split_*, the kernel k_split of sdr_split.hip)
against the integer model of tests/split_model.py. The definition is all integer, so every comparison
is byte for byte and every clip counter is compared exactly; there is no tolerance anywhere."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import scan_model as sm
import split_model as spm
import tuner_model as tm

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
# (mode, W, nwide, nblocks): every W, the history across blocks and the zero history of block 0, both
# batch positions; block_iq = 38400 is a whole number of 512-output workgroups and of 16-output tiles,
# 52920 and 73500 are neither
SHAPES = [(3, 4, 2, 3), (1, 8, 1, 2), (0, 10, 2, 2)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_RANDOM: dict = {}


def _random(shape):
    """(wide int8 [nblocks][nwide][2 W block_iq], the model's flipped sums): full-range random bytes
    with -128 certainly among them, made once and left unchanged."""
    if shape not in _RANDOM:
        mode, W, nwide, nblocks = shape
        n = 2 * W * spm.GEOM[mode][1]
        wide = np.random.default_rng(7000 + 10 * mode + W).integers(-128, 128, (nblocks, nwide, n), dtype=np.int8)
        wide[:, :, 5::997] = -128
        _RANDOM[shape] = (wide, spm.sums(mode, W, wide))
    return _RANDOM[shape]


def _gpu(pkg, torch, mode, W, wide, shift=None, pad_in=64, pad_out=32, sp=None):
    """(rows u8 [nblocks][nwide R][2 block_iq], clips [nwide][R]) of a fresh splitter (or sp) over the
    blocks. Input rows lie 2 W block_iq + pad_in bytes apart, output rows 2 block_iq + pad_out; the
    output padding must come back untouched."""
    nblocks, nwide, n = wide.shape
    own = sp is None
    if own:
        sp = pkg.Splitter(W, nwide, mode=mode, shift=shift)
    nb = 2 * sp.block_iq
    out = []
    for b in range(nblocks):
        hw = np.zeros((nwide, n + pad_in), np.int8)
        hw[:, :n] = wide[b]
        d = torch.from_numpy(hw).cuda()[:, :n]
        buf = torch.full((nwide * sp.rows, nb + pad_out), SENTINEL, dtype=torch.uint8, device="cuda")
        got = sp.block(d, out=buf[:, :nb])
        assert got.data_ptr() == buf.data_ptr()
        h = buf.cpu().numpy()
        assert np.all(h[:, nb:] == SENTINEL), f"block {b}: bytes past a row's end were written"
        out.append(h[:, :nb].copy())
    clips = sp.clips()
    if own:
        sp.close()
    return np.stack(out), clips


def _same(got, ref, what):
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at (block, row, byte) {bad[0].tolist()}: "
                             f"got {got[tuple(bad[0])]}, model {ref[tuple(bad[0])]}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "mode%d-W%d-n%d-b%d" % s)
def test_random_full_range(pkg, torch_cuda, shape):
    mode, W, nwide, nblocks = shape
    wide, acc = _random(shape)
    assert wide.min() == -128 and wide.max() == 127
    ref, ref_clips = spm.finish_all(acc, spm.SHIFT_DEFAULT[W])
    got, clips = _gpu(pkg, torch_cuda, mode, W, wide)
    _same(got, ref, f"shape {shape}")
    assert np.array_equal(clips, ref_clips)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "mode%d-W%d-n%d-b%d" % s)
def test_saturation(pkg, torch_cuda, shape):
    mode, W, nwide, nblocks = shape
    wide, acc = _random(shape)
    shift = spm.SHIFT_DEFAULT[W] - 4
    ref, ref_clips = spm.finish_all(acc, shift)
    v = 128 + ((acc + (1 << (shift - 1))) >> shift)
    assert (v < 0).any() and (v > 255).any() and (ref == 0).any() and (ref == 255).any()   # the model clips both ways
    assert ref_clips.min() > 0
    got, clips = _gpu(pkg, torch_cuda, mode, W, wide, shift=shift)
    _same(got, ref, f"shape {shape} shift {shift}")
    assert np.array_equal(clips, ref_clips)


def _extremes():
    """mode 3, W = 4, two blocks of five streams: all -128, all +127, and for rows 0, W - 1 and 2 W - 2 a
    stream of zeros with two windows whose bytes carry the signs of that row's acc_re tap column (127
    for positive, -128 for negative: |acc| is as large as it gets), one in the middle of block 0 and one
    straddling the boundary between blocks 0 and 1."""
    mode, W = 3, 4
    T, b = 16 * W, spm.GEOM[mode][1]
    M = spm.tap_matrix(W)
    s = np.zeros((5, 2 * 2 * W * b), np.int8)
    s[0] = -128
    s[1] = 127
    for i, r in enumerate((0, W - 1, 2 * W - 2)):
        pat = np.where(M[:, 2 * r] < 0, -128, 127).astype(np.int8)
        for t in (b // 2 + 3, b + 5):                               # W (b + 5) - T + 1 < W b: straddles
            s[2 + i, 2 * (W * t - T + 1):2 * (W * t + 1)] = pat
    return mode, W, np.ascontiguousarray(s.reshape(5, 2, 2 * W * b).transpose(1, 0, 2))


@pytest.mark.parametrize("shift", [24, 1])
def test_extremes(pkg, torch_cuda, shift):
    mode, W, wide = _extremes()
    acc = spm.sums(mode, W, wide)
    T = 16 * W
    for i, r in enumerate((0, W - 1, 2 * W - 2)):                   # the windows do reach the largest |acc|
        assert np.abs(acc[:, 2 + i, :, 2 * r]).max() >= 127 * np.abs(spm.tap_matrix(W)[:, 2 * r]).sum()
    assert np.abs(acc).max() < 2 ** 31 - 2 ** 23 and 2 * T * 128 * 8191 < 2 ** 31
    ref, ref_clips = spm.finish_all(acc, shift)
    got, clips = _gpu(pkg, torch_cuda, mode, W, wide, shift=shift)
    _same(got, ref, f"extremes shift {shift}")
    assert np.array_equal(clips, ref_clips)
    assert (ref_clips.sum() > 0) == (shift == 1)


def test_determinism_and_batch_independence(pkg, torch_cuda):
    shape = SHAPES[0]
    mode, W, nwide, nblocks = shape
    wide, acc = _random(shape)
    R = 2 * W - 1
    both, cb = _gpu(pkg, torch_cuda, mode, W, wide)
    again, ca = _gpu(pkg, torch_cuda, mode, W, wide)
    assert np.array_equal(both, again) and np.array_equal(cb, ca)
    swapped, cs = _gpu(pkg, torch_cuda, mode, W, np.ascontiguousarray(wide[:, ::-1]))
    assert np.array_equal(swapped[:, :R], both[:, R:]) and np.array_equal(swapped[:, R:], both[:, :R])
    assert np.array_equal(cs[::-1], cb)
    for w in range(nwide):
        alone, c1 = _gpu(pkg, torch_cuda, mode, W, np.ascontiguousarray(wide[:, w:w + 1]))
        assert np.array_equal(alone, both[:, w * R:(w + 1) * R]) and np.array_equal(c1[0], cb[w])
    # unpadded, 16-byte aligned rows give the same bytes as the padded ones
    plain, cp = _gpu(pkg, torch_cuda, mode, W, wide, pad_in=0, pad_out=0)
    assert np.array_equal(plain, both) and np.array_equal(cp, cb)
    # rows that are only 2-byte aligned (the C ABI asks no more) too
    odd, co = _gpu(pkg, torch_cuda, mode, W, wide, pad_out=6)
    assert np.array_equal(odd, both) and np.array_equal(co, cb)


def test_reset_and_refusals(pkg, torch_cuda):
    torch = torch_cuda
    shape = SHAPES[0]
    mode, W, nwide, nblocks = shape
    wide, acc = _random(shape)
    shift = spm.SHIFT_DEFAULT[W] - 4                                # clips, so the counters matter
    ref, ref_clips = spm.finish_all(acc, shift)
    sp = pkg.Splitter(W, nwide, mode=mode, shift=shift)
    _gpu(pkg, torch, mode, W, wide[:2], sp=sp)                      # history and counters now non-zero
    sp.reset()
    assert not sp.clips().any()
    # a refused call enqueues nothing: neither the rows, nor the history, nor the counters move
    n, nb = wide.shape[2], 2 * sp.block_iq
    d = torch.from_numpy(wide[1]).cuda()
    buf = torch.full((nwide * sp.rows, nb), SENTINEL, dtype=torch.uint8, device="cuda")
    L, E = pkg.lib(), -1
    st = None
    assert L.sdr_split_block(sp._h, d.data_ptr(), n - 4, buf.data_ptr(), nb, st) == E       # short wide stride
    assert L.sdr_split_block(sp._h, d.data_ptr(), n + 2, buf.data_ptr(), nb, st) == E       # no multiple of 4
    assert L.sdr_split_block(sp._h, d.data_ptr() + 2, n, buf.data_ptr(), nb, st) == E       # wide misaligned
    assert L.sdr_split_block(sp._h, d.data_ptr(), n, buf.data_ptr(), nb - 2, st) == E       # short row stride
    assert L.sdr_split_block(sp._h, d.data_ptr(), n, buf.data_ptr(), nb + 1, st) == E       # odd row stride
    assert L.sdr_split_block(sp._h, d.data_ptr(), n, buf.data_ptr() + 1, nb + 2, st) == E   # odd rows address
    assert L.sdr_split_block(sp._h, None, n, buf.data_ptr(), nb, st) == E
    assert L.sdr_split_block(sp._h, d.data_ptr(), n, None, nb, st) == E
    assert L.sdr_split_clips(sp._h, None, st) == E
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    got, clips = _gpu(pkg, torch, mode, W, wide, sp=sp)
    sp.close()
    _same(got, ref, "after reset and refused calls")
    assert np.array_equal(clips, ref_clips)
    h = C.c_void_p()
    for args in ((4, 4, 1, 0), (0, 5, 1, 0), (0, 4, 0, 0), (0, 4, 1, 25)):
        assert L.sdr_split_create(C.byref(h), 0, *args) == E and not h.value


COMPOSITION_KHZ = (-7500, 200, 6900)


def test_composition_scan_and_tuner(pkg, oracle, synth, torch_cuda):
    """Mode 0, W = 8, 2 blocks, stations at -7500, +200 and +6900 kHz of the wide capture: Splitter ->
    Scanner on all 15 rows -> the wide picker finds exactly the three; then the tuner on the split rows
    gives the fm_demod of the model's rows bit for bit."""
    torch = torch_cuda
    mode, W, nblocks = 0, 8, 2
    R = 2 * W - 1
    wide1, clipped = spm.wide_composite(synth, W, nblocks, COMPOSITION_KHZ)
    assert clipped == 0
    wide = wide1[:, None, :]
    ref, ref_clips = spm.run(mode, W, wide)
    assert not ref_clips.any()
    expect = [(1, -300), (7, 200), (13, -300)]
    # the model's rows through the scan's model: the same three, nothing in the other 12 rows
    A, _tol, S = sm.rows_power(pkg, mode, [ref[b] for b in range(nblocks)])
    assert spm.wide_pick(mode, W, (A / S).astype(np.float32), sm.pick) == expect
    sp, sc = pkg.Splitter(W, 1, mode=mode), pkg.Scanner(mode, R)
    d = torch.from_numpy(wide).cuda()
    rows = [sp.block(d[b]) for b in range(nblocks)]
    for r in rows:
        sc.block(r)
    psd, seg = sc.psd()
    assert seg == S
    assert not sp.clips().any()
    _same(np.stack([r.cpu().numpy() for r in rows]), ref, "composite")

    def lib_pick(row, **o):
        return pkg.scan_pick(mode, row, **o)

    found = spm.wide_pick(mode, W, psd, lib_pick)
    assert found == expect
    # the three rows lie 6 apart: a strided view of the split rows is the tuner's capture batch as it stands
    src, khz = [s for s, _ in found], [k for _, k in found]
    assert src == [1, 7, 13]
    pipe = pkg.Pipeline(3, mode=mode, rds_on=True, device=0)
    pipe.set_tuning([0, 1, 2], khz, 3)
    want = tm.run_tuned(pkg, oracle, mode, ref[:, 1::6], [0, 1, 2], khz)
    for b in range(nblocks):
        pipe.frontend_tuned(rows[b][1::6])
        fm = pipe.fm_demod().cpu().numpy()
        for c in range(3):
            assert np.array_equal(fm[c].view(np.uint32), want[c]["fm"][b].view(np.uint32)), f"fm_demod block {b} ch {c}"
    pipe.close()
    sc.close()
    sp.close()
