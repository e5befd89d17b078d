"""GPU: the band scan (include/sdr_amd.h: sdr_scan_*, the kernel k_scan_psd of sdr_scan.hip) against
the f64 model of tests/scan_model.py, one block of 3-8 rows per test.

Tolerance (derived, not measured): per bin, with A_ref[k] = sum_s |X_ref,s[k]|^2 over the S segments,
    tol[k] = sum_s (2 |X_ref,s[k]| e_s + e_s^2) + (S + 6) 2^-24 A_ref[k],   e_s = 2^-16 sum_n |xw_n|.
The first-order worst-case error of a mixed-radix f32 DFT built as the header says is
(sum of the radices + 8) 2^-24 ||xw||_1 -- 98 + 8 for 48 x 50, 76 + 8 for 36 x 40, 68 + 8 for 32 x 36;
the + 8 covers the window product, the twiddle products and the table's own rounding -- and
2^-16 = 256 2^-24 leaves 2.4 times that for the largest; the last term is the f32 accumulation of the
S powers and the division by S."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

import scan_model as sm
import tuner_model as tm
from conftest import ROOT

pytestmark = pytest.mark.gpu

RADICES = {0: (48, 50), 1: (36, 40), 2: (48, 50), 3: (32, 36)}   # k_scan_psd's factorisation per mode


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


_RANDOM: dict = {}


def _random_rows(pkg, mode, nrows=3):
    """(rows u8 [nrows][2*block_iq], A_ref, tol, S): uniform random bytes and their model, made once."""
    if mode not in _RANDOM:
        block_iq = pkg.scan_geometry(mode)[2]
        rows = np.random.default_rng(100 + mode).integers(0, 256, (nrows, 2 * block_iq), dtype=np.uint8)
        _RANDOM[mode] = (rows,) + sm.rows_power(pkg, mode, [rows])
    return _RANDOM[mode]


def _scan(pkg, torch, mode, blocks, pad=0):
    """(psd, segments) of a fresh scanner over blocks (each u8 [nrows][2*block_iq]); pad > 0: the rows
    lie pad bytes apart more than their length."""
    sc = pkg.Scanner(mode, blocks[0].shape[0])
    for blk in blocks:
        if pad:
            wide = np.zeros((blk.shape[0], blk.shape[1] + pad), np.uint8)
            wide[:, :blk.shape[1]] = blk
            d = torch.from_numpy(wide).cuda()[:, :blk.shape[1]]
            assert d.stride(0) == blk.shape[1] + pad
        else:
            d = torch.from_numpy(np.ascontiguousarray(blk)).cuda()
        sc.block(d)
    out = sc.psd()
    sc.close()
    return out


def _check(psd, S, A_ref, tol, what):
    err = np.abs(S * psd.astype(np.float64) - A_ref)
    worst = float((err / tol).max())
    print(f"{what}: worst |S psd - A_ref| / tol = {worst:.4f}, worst error / largest bin {float(err.max() / A_ref.max()):.3e}")
    assert np.all(err <= tol), f"{what}: {int((err > tol).sum())} bins over the tolerance, worst {worst:.3f} x tol"


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_accuracy_random_rows(pkg, torch_cuda, mode):
    """3 rows of uniform random bytes; mode 0's rows lie 2*block_iq + 64 bytes apart, so rows 0 and 2
    start 16-byte aligned and row 1 does not (the kernel's two load paths)."""
    rows, A_ref, tol, S = _random_rows(pkg, mode)
    psd, seg = _scan(pkg, torch_cuda, mode, [rows], pad=64 if mode == 0 else 0)
    assert seg == S == pkg.scan_geometry(mode)[1]
    assert psd.shape == A_ref.shape and psd.dtype == np.float32
    _check(psd, S, A_ref, tol, f"mode {mode}")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_tones_bin_order_and_sign(pkg, torch_cuda, mode):
    """One row per tone e^(+j 2 pi k0 n / N): the peak is bin k0 mod N, which is tuner offset khz = k0."""
    N, S, block_iq = pkg.scan_geometry(mode)
    k0s = [0, 1, -1, N // 2, 37, -301 if N == 1152 else -601] + list(RADICES[mode])
    rows = np.empty((len(k0s), 2 * block_iq), np.uint8)
    for r, k0 in enumerate(k0s):
        z = 127.0 * 0.9 * np.exp(2j * np.pi * ((k0 * np.arange(block_iq, dtype=np.int64)) % N) / N)
        rows[r, 0::2] = np.round(z.real + 128.0)
        rows[r, 1::2] = np.round(z.imag + 128.0)
    A_ref, tol, S_m = sm.rows_power(pkg, mode, [rows])
    psd, seg = _scan(pkg, torch_cuda, mode, [rows])
    assert seg == S_m == S
    _check(psd, S, A_ref, tol, f"mode {mode} tones")
    for r, k0 in enumerate(k0s):
        assert int(np.argmax(psd[r])) == k0 % N, f"k0 {k0}"
        khz, db = pkg.scan_pick(mode, psd[r], step_khz=1, half_width_khz=0, sep_khz=2, guard_khz=0)
        # (k0 = N/2: with guard 0 the candidates -N/2 and N/2 name the same bin and tie; -N/2 comes first)
        assert khz.size >= 1 and (int(khz[0]) - k0) % N == 0, f"k0 {k0}: picked {khz[:4]}"
        if 2 * abs(k0) < N:
            assert int(khz[0]) == k0, f"k0 {k0}: picked {khz[:4]}"


def test_determinism_and_batch_independence(pkg, torch_cuda):
    rows = _random_rows(pkg, 0)[0]
    alone, _ = _scan(pkg, torch_cuda, 0, [rows[2:3]])
    batch, _ = _scan(pkg, torch_cuda, 0, [rows])
    again, _ = _scan(pkg, torch_cuda, 0, [rows])
    assert np.array_equal(_u32(alone[0]), _u32(batch[2])), "a row's spectrum depends on the rows beside it"
    assert np.array_equal(_u32(batch), _u32(again)), "two runs differ"
    other = np.ascontiguousarray(rows[::-1])
    swapped, _ = _scan(pkg, torch_cuda, 0, [other])
    assert np.array_equal(_u32(swapped[0]), _u32(batch[2])) and np.array_equal(_u32(swapped[2]), _u32(batch[0]))


def test_accumulation_and_reset(pkg, torch_cuda):
    torch = torch_cuda
    mode = 1
    rows, _, _, S_b = _random_rows(pkg, mode)
    second = np.ascontiguousarray(np.roll(rows, 12345, axis=1)[::-1])
    A_ref, tol, S = sm.rows_power(pkg, mode, [rows, second])
    d1, d2 = torch.from_numpy(rows).cuda(), torch.from_numpy(second).cuda()
    sc = pkg.Scanner(mode, 3)
    psd0, seg0 = sc.psd()
    assert seg0 == 0 and not psd0.any()
    sc.block(d1)
    sc.block(d2)
    psd, seg = sc.psd()
    assert seg == S == 2 * S_b
    _check(psd, S, A_ref, tol, "two blocks")
    sc.reset()
    sc.block(d1)
    after, seg1 = sc.psd()
    sc.close()
    fresh, seg2 = _scan(pkg, torch, mode, [rows])
    assert seg1 == seg2 == S_b
    assert np.array_equal(_u32(after), _u32(fresh)), "reset() left something behind"


def test_end_to_end_scan_then_tune(pkg, oracle, synth, torch_cuda):
    """The composite capture: the scan finds its three stations, and what it returns is valid tuner
    input -- the tuned front end on it equals the tuner's CPU model bit for bit."""
    torch = torch_cuda
    comp = tm.composite(synth, 2)[0]                               # [2 blocks][bytes]
    d = torch.from_numpy(np.ascontiguousarray(comp[:, None, :])).cuda()
    sc = pkg.Scanner(0, 1)
    for b in range(2):
        sc.block(d[b])
    src, khz = sc.stations()
    _, seg = sc.psd()
    sc.close()
    assert seg == 60
    assert src.dtype == np.int32 and khz.dtype == np.int32
    assert src.tolist() == [0, 0, 0] and sorted(khz.tolist()) == [-600, 0, 500], (src, khz)
    pipe = pkg.Pipeline(3)
    pipe.set_tuning(src, khz)
    pipe.frontend_tuned(d[0])
    fm = pipe.fm_demod().cpu().numpy()
    pipe.close()
    want = tm.run_tuned(pkg, oracle, 0, comp[:1, None, :], src.tolist(), khz.tolist())
    for c in range(3):
        assert np.array_equal(_u32(fm[c]), _u32(want[c]["fm"][0])), f"station {khz[c]} kHz"


def test_refusals(pkg, torch_cuda):
    torch = torch_cuda
    L = pkg.lib()
    h = C.c_void_p()
    for mode, nsrc in ((4, 1), (-1, 1), (0, 0), (0, -3)):
        assert L.sdr_scan_create(C.byref(h), 0, mode, nsrc) == -1 and not h.value, (mode, nsrc)
    assert L.sdr_scan_create(None, 0, 0, 1) == -1
    with pytest.raises(pkg.SdrError) as e:
        pkg.Scanner(7, 1)
    assert e.value.code == -1
    block_iq = pkg.scan_geometry(0)[2]
    rows = _random_rows(pkg, 0)[0]
    d = torch.from_numpy(rows).cuda()
    sc = pkg.Scanner(0, 3)
    st = pkg._stream()
    assert L.sdr_scan_block(sc._h, None, 2 * block_iq, st) == -1                        # NULL iq
    assert L.sdr_scan_block(sc._h, d.data_ptr(), 2 * block_iq - 2, st) == -1            # short stride
    assert L.sdr_scan_block(sc._h, d.data_ptr(), 2 * block_iq + 1, st) == -1            # odd stride
    assert L.sdr_scan_block(sc._h, d.data_ptr() + 1, 2 * block_iq, st) == -1            # odd address
    assert L.sdr_scan_block(None, d.data_ptr(), 2 * block_iq, st) == -1
    assert L.sdr_scan_psd(sc._h, None, None, st) == -1 and L.sdr_scan_reset(None, st) == -1
    with pytest.raises(pkg.SdrError):
        sc.block(d[:2])                                                                 # 2 rows for a 3-row scanner
    psd, seg = sc.psd()
    assert seg == 0 and not psd.any(), "a refused call enqueued something"
    sc.block(d)                                                                         # and it still works
    assert sc.psd()[1] == 30
    sc.close()


def test_cli_scan_then_tune(pkg, synth, tmp_path):
    exe = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"
    assert exe.exists(), "build with make"
    tm.composite(synth, 2)[0].tofile(tmp_path / "in.u8")           # [block][1 row][bytes]
    r = subprocess.run([str(exe), "1", "--scan", "--in", str(tmp_path / "in.u8"), "--out", str(tmp_path / "rx")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "sdr_multi: scan: 3 stations in 1 rows (60 segments per row)" in r.stderr, r.stderr
    lines = (tmp_path / "rx.stations").read_text().splitlines()
    assert sorted(lines) == sorted(f"0 {k}" for k in tm.COMPOSITE_KHZ), lines
    r = subprocess.run([str(exe), "3", "--tune", str(tmp_path / "rx.stations"), "--cus", "16", "--in",
                        str(tmp_path / "in.u8"), "--out", str(tmp_path / "rx")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert "3 channels" in r.stderr and "x 2 blocks" in r.stderr, r.stderr
    # --scan together with --tune is a usage error
    r = subprocess.run([str(exe), "1", "--scan", "--tune", str(tmp_path / "rx.stations"), "--in",
                        str(tmp_path / "in.u8")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stderr, r.stderr
