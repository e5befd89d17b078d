"""GPU: the fast front end (SDR_FLAG_FAST_FRONTEND: k_frontend_mfma and ft_tile_iq of sdr_frontend.hip)
sample by sample against the f64 definition, within the tolerance derived in tests/fast_fe_model.py
(its docstring holds the derivation; tests/test_fast_fe_model.py shows on the CPU that the tolerance
leaves the defect-free arithmetic half its room and that five subtle defects exceed it).

Every test builds pkg.Pipeline(nch, mode=mode, flags=pkg.FLAG_FAST_FRONTEND), runs frontend() and reads
fm_demod() block by block: block 0 has the u8-128 history, block 1 the previous block's tail, block 2
the first reuse of a parity. Rows are passed 16-byte aligned with a 16-byte stride (the dwordx4 staging,
X4) and with a stride of 8 mod 16 (the 8-byte staging; mode 0's plain row, 147000 bytes, is one)."""
from __future__ import annotations

import numpy as np
import pytest

import fast_fe_model as fm

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2, 3)                 # D = 10, 4, 10, 3; block_if 7350, 13230, 8000, 12800
LAYOUTS = ("x4", "8B")
NBLOCKS = 3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _device_rows(torch, rows, layout):
    """rows u8 [nblocks][nch][row] on the device, one [nch][row] view per block: "x4" 16-byte aligned rows
    (stride a multiple of 16), "8B" 8-byte aligned rows whose stride is 8 mod 16."""
    nb, nch, row = rows.shape
    stride = (row + 15) // 16 * 16
    if layout == "8B":
        stride = (row + 7) // 8 * 8
        stride += 8 if stride % 16 == 0 else 0
    out = []
    for b in range(nb):
        d = torch.full((nch, stride), 7, dtype=torch.uint8, device="cuda")[:, :row]    # the padding is not 128
        d.copy_(torch.from_numpy(np.ascontiguousarray(rows[b])))
        assert d.stride(0) == stride and d.data_ptr() % 16 == 0 and (stride % 16 == 0) == (layout == "x4")
        out.append(d)
    return out


def _feed(pipe, blocks):
    got = []
    for d in blocks:
        pipe.frontend(d)
        got.append(pipe.fm_demod().cpu().numpy())
    return np.stack(got)


def _run(pkg, torch, rows, mode, layout):
    """fm_demod f32 [nblocks][nch][block_if] of a fresh fast context over rows."""
    pipe = pkg.Pipeline(rows.shape[1], mode=mode, flags=pkg.FLAG_FAST_FRONTEND)
    got = _feed(pipe, _device_rows(torch, rows, layout))
    pipe.close()
    return got


_KINDS: dict = {}
_GOT: dict = {}
_EXTREMES: dict = {}


def _kinds(torch, synth, oracle, mode):
    """One channel per synth.KINDS at the mode's rf_Fs, generated on the device and copied back, with the
    f64 truth and the tolerance of exactly those bytes; made once per mode."""
    if mode not in _KINDS:
        g = fm.geometry(oracle, mode)
        src = synth.TorchMultiplexBatch(torch, len(synth.KINDS), kinds=synth.KINDS, seed=5 + mode, fs=g["fs"])
        rows = np.stack([src.next_block(g["block_iq"]).cpu().numpy() for _ in range(NBLOCKS)])
        t = fm.truth(mode, rows, oracle)
        _KINDS[mode] = {"rows": rows, "t": t, "tol": fm.tol(t)}
    return _KINDS[mode]


def _kinds_gpu(pkg, torch, synth, oracle, mode, layout):
    if (mode, layout) not in _GOT:
        _GOT[mode, layout] = _run(pkg, torch, _kinds(torch, synth, oracle, mode)["rows"], mode, layout)
    return _GOT[mode, layout]


def _check(got, t, tol, names, what):
    """Every sample within tol; +0 exactly where tol is 0. Prints the worst ratio per row."""
    r = fm.ratio(got, t, tol)
    for j, name in enumerate(names):
        print(f"GPU {what} {name}: worst err/tol {r[:, j].max():.3f}")
    bad = np.argwhere(r > 1.0)
    assert bad.size == 0, (f"{what}: {len(bad)} samples over tol, first (block, row, output) {tuple(bad[0])} "
                           f"of {names[bad[0][1]]}: ratio {r[tuple(bad[0])]:.3f}")
    z = tol == 0
    assert not _u32(got[z]).any(), f"{what}: not +0 where the taps meet only u8 128"
    return r


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
def test_every_kind_every_mode(pkg, synth, oracle, torch_cuda, mode, layout):
    """a. The eleven synth.KINDS, one channel each, three blocks: |fm_demod - truth| <= tol on every sample;
    silence is +0 in every sample; rail is +0, bit-equal to the oracle, once the window has left the history."""
    k = _kinds(torch_cuda, synth, oracle, mode)
    got = _kinds_gpu(pkg, torch_cuda, synth, oracle, mode, layout)
    names = list(synth.KINDS)
    _check(got, k["t"], k["tol"], names, f"mode {mode} {layout}")
    assert not _u32(got[:, names.index("silence")]).any()
    j = names.index("rail")
    ch = oracle.Channel(mode, True)
    ref = np.stack([ch.frontend(k["rows"][b, j]) for b in range(NBLOCKS)])
    s0 = fm.steady_from(fm.geometry(oracle, mode)["D"])
    for b in range(NBLOCKS):
        lo = s0 if b == 0 else 0
        assert not _u32(got[b, j, lo:]).any(), f"rail block {b}: not +0 in steady state"
        assert np.array_equal(_u32(got[b, j, lo:]), _u32(ref[b, lo:])), f"rail block {b} vs the oracle"
    # block 1, output 0: the previous sample is the last of block 0 (prev_in), not (0, 0)
    r0 = fm.ratio(got, k["t"], k["tol"])[1, :, 0]
    assert np.all(r0 <= 1.0) and np.isfinite(k["tol"][1, names.index("normal"), 0])
    assert k["tol"][1, names.index("normal"), 0] < 0.01 * np.abs(k["t"]["q"][1, names.index("normal")]).max()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_extremes(pkg, oracle, torch_cuda, mode, layout):
    """b. D = 10, 4, 3: every byte 0 (int8 -128 on every operand), every byte 255, samples alternating 0 and
    255, and three full-scale tap-signed windows (mid block, across blocks 0 / 1, across the first tile
    boundary) whose |y| is the largest the taps allow: the int32 digit pairing at its widest."""
    g = fm.geometry(oracle, mode)
    if mode not in _EXTREMES:
        rows = fm.extremes(oracle, mode, NBLOCKS)
        t = fm.truth(mode, rows, oracle)
        margins: dict = {}
        fm.kernel_model(mode, rows, oracle, margins=margins)
        _EXTREMES[mode] = (rows, t, fm.tol(t), margins)
    rows, t, tol, margins = _EXTREMES[mode]
    sum_h = np.abs(g["h"].astype(np.float64)).sum()
    for name, out in fm.extreme_outputs(oracle, mode).items():        # on the model first
        j = fm.EXTREME_ROWS.index(name)
        b, n = divmod(out, g["block_if"])
        assert min(abs(t["cI"][b, j, n]), abs(t["cQ"][b, j, n])) >= 127 / 128 * sum_h
    assert max(margins.values()) < 2 ** 31 and margins["pair_lo"] > 2 ** 24        # the conversions do round here
    assert (margins["pair"] > 2 ** 24) == (t["F"] == 33)                           # (float)hI: at F = 33 (D = 10)
    got = _run(pkg, torch_cuda, rows, mode, layout)
    _check(got, t, tol, list(fm.EXTREME_ROWS), f"extremes mode {mode} {layout}")
    s0 = fm.steady_from(g["D"])
    for j in range(3):                                                # I = Q throughout: the quotient is +0
        assert not _u32(got[0, j, s0:]).any() and not _u32(got[1:, j]).any(), fm.EXTREME_ROWS[j]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
def test_named_edges(pkg, synth, oracle, torch_cuda, mode, layout):
    """c. err / tol at the outputs where the kernel changes path, named: 0 and 1 of each block (prev_in, the
    history or tail), ADV - 1, ADV, ADV + 1 (the first tile boundary: the carry rows), the last tile's first
    output and block_if - 1 (prev_out, the padding past the block)."""
    g = fm.geometry(oracle, mode)
    k = _kinds(torch_cuda, synth, oracle, mode)
    got = _kinds_gpu(pkg, torch_cuda, synth, oracle, mode, layout)
    r = fm.ratio(got, k["t"], k["tol"])
    ADV, nif = fm.adv(g["D"]), g["block_if"]
    edges = {"0": 0, "1": 1, "ADV-1": ADV - 1, "ADV": ADV, "ADV+1": ADV + 1,
             "last tile's first": (nif - 1) // ADV * ADV, "block_if-1": nif - 1}
    checked = [j for j, name in enumerate(synth.KINDS) if name not in ("silence", "rail")]
    for b in range(NBLOCKS):
        for name, n in edges.items():
            worst = r[b, :, n].max()
            print(f"GPU mode {mode} {layout} block {b} output {name} ({n}): worst err/tol {worst:.3f}")
            assert worst <= 1.0, f"mode {mode} {layout} block {b} output {name} ({n}): {worst:.3f}"
            if (b, n) != (0, 0):           # there the only sample past the history meets h[0] = 0: c = 0, q = 0
                assert np.all(np.isfinite(k["tol"][b, checked, n])), f"output {name}: an ill-posed sample"


@pytest.mark.parametrize("mode", [0, 3])
def test_layout_and_batch_independence(pkg, synth, oracle, torch_cuda, mode):
    """d. A row's fm_demod has the same bits through the X4 and the 8-byte staging, alone, as channel 63, 64
    or 66 of 67, and with the batch order reversed (two blocks)."""
    torch = torch_cuda
    g = fm.geometry(oracle, mode)
    nch = 67
    kinds = [synth.KINDS[c % len(synth.KINDS)] for c in range(nch)]
    src = synth.TorchMultiplexBatch(torch, nch, kinds=kinds, seed=23 + mode, fs=g["fs"])
    rows = np.stack([src.next_block(g["block_iq"]).cpu().numpy() for _ in range(2)])
    base = _run(pkg, torch, rows, mode, "x4")
    assert np.array_equal(_u32(base), _u32(_run(pkg, torch, rows, mode, "8B"))), "X4 vs 8-byte staging"
    rev = _run(pkg, torch, np.ascontiguousarray(rows[:, ::-1]), mode, "x4")
    assert np.array_equal(_u32(base), _u32(rev[:, ::-1])), "batch order reversed"
    for c in (0, 63, 64, 66):
        for layout in LAYOUTS:
            alone = _run(pkg, torch, rows[:, c:c + 1], mode, layout)
            assert np.array_equal(_u32(alone[:, 0]), _u32(base[:, c])), f"row {c} alone ({layout}) vs in the batch"


@pytest.mark.parametrize("mode", [0, 3])
def test_state(pkg, synth, oracle, torch_cuda, mode):
    """e. reset() on a fast context: after an odd number of other blocks and a reset, blocks 0 to 2 come out
    bit-identical to a fresh context's. Two contexts alive at once on different bytes do not disturb each other."""
    torch = torch_cuda
    k = _kinds(torch, synth, oracle, mode)
    rows, other = k["rows"], np.ascontiguousarray(k["rows"][:, ::-1])
    fresh = _kinds_gpu(pkg, torch, synth, oracle, mode, "x4")
    fresh_other = _run(pkg, torch, other, mode, "x4")
    d_rows, d_other = _device_rows(torch, rows, "x4"), _device_rows(torch, other, "x4")
    pipe = pkg.Pipeline(rows.shape[1], mode=mode, flags=pkg.FLAG_FAST_FRONTEND)
    assert np.array_equal(_u32(_feed(pipe, d_other)), _u32(fresh_other))
    pipe.reset()
    assert np.array_equal(_u32(_feed(pipe, d_rows)), _u32(fresh)), "after reset()"
    pipe.reset()
    pa = pipe
    pb = pkg.Pipeline(rows.shape[1], mode=mode, flags=pkg.FLAG_FAST_FRONTEND)
    for b in range(NBLOCKS):
        pa.frontend(d_rows[b])
        pb.frontend(d_other[b])
        ga, gb = pa.fm_demod().cpu().numpy(), pb.fm_demod().cpu().numpy()
        assert np.array_equal(_u32(ga), _u32(fresh[b])), f"context A block {b}"
        assert np.array_equal(_u32(gb), _u32(fresh_other[b])), f"context B block {b}"
    pa.close()
    pb.close()
