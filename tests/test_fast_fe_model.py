"""CPU: the models of tests/fast_fe_model.py checked against each other and against the oracle, on the
inputs tests/test_gpu_fast_frontend.py runs on the GPU. This file is the evidence that the GPU test can
fail: the defect-free kernel model sits at most at half the derived tolerance, the f32 reference sits
within the same form with its own FIR bound, the tolerance is small against the signal on all but a
per cent of the samples, and each of five subtle defects of the kernel exceeds it somewhere.

Inputs: the eleven synth.KINDS, one channel each, from synth.TorchMultiplexBatch on the CPU device at the
mode's rf_Fs (the GPU test generates them on the device: other bytes, the same kinds), and the extreme
rows of fast_fe_model.extremes(); three blocks each.

Blocks whose f64 fm_demod is identically 0 although the samples are not (every byte 255 or 0, or I = Q
throughout, once the window has left the history) have no scale to compare a tolerance with; there the
kernel model must give +0 in every sample, which is the stronger statement, and the informativeness
condition is taken over the other blocks."""
from __future__ import annotations

import numpy as np
import pytest

import fast_fe_model as fm

KIND_MODES = (0, 1, 2, 3)            # D = 10, 4, 10, 3
EXTREME_MODES = (0, 1, 3)            # D = 10, 4, 3
NBLOCKS = 3
CASES = [("kinds", m) for m in KIND_MODES] + [("extremes", m) for m in EXTREME_MODES]
CASE_IDS = [f"{s}_mode{m}" for s, m in CASES]

_CASE: dict = {}


def _rows(synth, oracle, which, mode):
    g = fm.geometry(oracle, mode)
    if which == "extremes":
        return fm.extremes(oracle, mode, NBLOCKS), fm.EXTREME_ROWS
    import torch
    src = synth.TorchMultiplexBatch(torch, len(synth.KINDS), device="cpu", kinds=synth.KINDS, seed=11 + mode,
                                    fs=g["fs"])
    return np.stack([src.next_block(g["block_iq"]).numpy().copy() for _ in range(NBLOCKS)]), synth.KINDS


def case(synth, oracle, which, mode):
    """rows, row names, truth, tolerance and the defect-free kernel model of one input set, made once."""
    key = (which, mode)
    if key not in _CASE:
        rows, names = _rows(synth, oracle, which, mode)
        t = fm.truth(mode, rows, oracle)
        margins: dict = {}
        _CASE[key] = {"rows": rows, "names": names, "t": t, "tol": fm.tol(t), "margins": margins,
                      "model": fm.kernel_model(mode, rows, oracle, margins=margins)}
    return _CASE[key]


def test_tap_digits(oracle):
    for mode in KIND_MODES:
        h = fm.geometry(oracle, mode)["h"]
        F, H, dig = fm.tap_digits(h)
        assert np.abs(H).max() < 2 ** 30 and np.abs(H).max() >= 2 ** 28            # |h 2^F| in [2^29, 2^30) before rounding
        assert np.max(np.abs(H * 2.0 ** -F - h.astype(np.float64))) <= 2.0 ** -(F + 1)
        assert h[0] == 0.0 and H[fm.TAP_SHIFT_TAP] != H[fm.TAP_SHIFT_TAP - 1]       # the tap_shift defect changes a tap


@pytest.mark.parametrize("which,mode", CASES, ids=CASE_IDS)
def test_model_within_half_tol(synth, oracle, which, mode):
    c = case(synth, oracle, which, mode)
    r = fm.ratio(c["model"], c["t"], c["tol"])
    for j, name in enumerate(c["names"]):
        print(f"{which} mode {mode} {name}: worst model err/tol {r[:, j].max():.3f}")
    assert r.max() <= 0.5, f"{which} mode {mode}: {r.max():.3f}"
    # exact zeros: the taps meet only u8 128
    z = c["tol"] == 0
    assert np.array_equal(c["model"][z].view(np.uint32), np.zeros(int(z.sum()), np.uint32))
    if which == "kinds":
        assert z[:, c["names"].index("silence")].all()


@pytest.mark.parametrize("which,mode", CASES, ids=CASE_IDS)
def test_oracle_within_its_bound(synth, oracle, which, mode):
    """The f32 reference against the same truth, with the sequential FIR's own bound for e."""
    c = case(synth, oracle, which, mode)
    tol_ref = fm.tol(c["t"], reference=True)
    for j, name in enumerate(c["names"]):
        ch = oracle.Channel(mode, True)
        got = np.stack([ch.frontend(c["rows"][b, j]) for b in range(NBLOCKS)])
        t = fm.rows_of(c["t"], j)
        r = fm.ratio(got[:, None, :], t, tol_ref[:, j:j + 1])
        print(f"{which} mode {mode} {name}: worst oracle err/tol_ref {r.max():.3f}")
        assert r.max() <= 1.0, f"{which} mode {mode} {name}: {r.max():.3f}"
        z = tol_ref[:, j] == 0
        assert not got[z].any()


@pytest.mark.parametrize("which,mode", CASES, ids=CASE_IDS)
def test_tolerance_is_informative(synth, oracle, which, mode):
    """tol <= 1 % of the block's largest |q| on at least 99 % of the samples of every row but silence."""
    c = case(synth, oracle, which, mode)
    for j, name in enumerate(c["names"]):
        if name == "silence":
            continue
        for b in range(NBLOCKS):
            qmax = np.abs(c["t"]["q"][b, j]).max()
            if qmax == 0.0:                                  # q = 0 throughout: the model must say +0
                assert not c["model"][b, j].view(np.uint32).any(), f"{name} block {b}"
                assert name in ("rail", "all_0", "all_255", "alternating") or not c["tol"][b, j].any()
                continue
            share = np.mean(c["tol"][b, j] > 0.01 * qmax)
            print(f"{which} mode {mode} {name} block {b}: share of samples with tol > 1% max|q| {share:.4f}")
            assert share <= 0.01, f"{which} mode {mode} {name} block {b}: {share:.4f}"


# which input set catches which defect (every entry is asserted; the first is the subtlest input that does)
CATCHES = {
    "three_planes": [("kinds", 0, "noise"), ("kinds", 3, "noise")],
    "two_planes": [("kinds", 0, "normal"), ("kinds", 0, "weak"), ("extremes", 0, "window_mid")],
    "tap_shift": [("kinds", 0, "normal"), ("kinds", 1, "saturated")],
    "carry": [("kinds", 0, "normal"), ("kinds", 3, "weak")],
    "prev0": [("kinds", 0, "normal"), ("kinds", 1, "carrier_offset")],
}


@pytest.mark.parametrize("defect", fm.DEFECTS)
def test_defect_exceeds_tol(synth, oracle, defect):
    for which, mode, name in CATCHES[defect]:
        c = case(synth, oracle, which, mode)
        j = c["names"].index(name)
        bad = fm.kernel_model(mode, c["rows"][:, j:j + 1], oracle, defect=defect)
        t = fm.rows_of(c["t"], j)
        r = fm.ratio(bad, t, c["tol"][:, j:j + 1])
        print(f"{defect} on {which} mode {mode} {name}: worst err/tol {r.max():.2f}, {int((r > 1).sum())} samples over")
        assert r.max() > 1.0, f"{defect} not caught on {which} mode {mode} {name}: {r.max():.3f}"
        if defect == "prev0":                                # only output 0 of blocks 1 and 2 can differ
            assert np.all(r[0] <= 1.0) and np.all(r[1:, :, 1:] <= 1.0) and np.all(r[1:, :, 0] > 1.0)


@pytest.mark.parametrize("mode", EXTREME_MODES)
def test_extremes_reach_the_int32_range(synth, oracle, mode):
    """The tap-signed windows reach the largest |y| the taps allow, and the int32 sums of ft_tile_iq keep
    their headroom there."""
    c = case(synth, oracle, "extremes", mode)
    g = fm.geometry(oracle, mode)
    sum_h = np.abs(g["h"].astype(np.float64)).sum()
    nif = g["block_if"]
    for name, out in fm.extreme_outputs(oracle, mode).items():
        j = c["names"].index(name)
        b, n = divmod(out, nif)
        assert abs(c["t"]["cI"][b, j, n]) >= 127 / 128 * sum_h and abs(c["t"]["cQ"][b, j, n]) >= 127 / 128 * sum_h
        assert c["t"]["AI"][b, j, n] >= 127 / 128 * sum_h
    m = c["margins"]
    print(f"D {g['D']}: largest |plane sum| {m['plane']} = 2^31 / {2 ** 31 / m['plane']:.1f}, "
          f"largest |(a0 << 8) + a1| {m['pair']} = 2^31 / {2 ** 31 / m['pair']:.2f}, "
          f"largest |(a2 << 8) + a3| {m['pair_lo']} = 2^31 / {2 ** 31 / m['pair_lo']:.2f}")
    assert max(m["plane"], m["pair"], m["pair_lo"]) < 2 ** 31
    # the high pair is at least the quantised full-scale sum's high half: the windows do exercise it
    F = c["t"]["F"]
    assert m["pair"] >= (int(127 * sum_h * 2.0 ** F) >> 16) - 2 ** 14       # |lI| < 2^30: at most 2^14 of hI
    # (float)hI rounds only past 2^24: it does at F = 33 (D = 10), not at F = 32 (D = 4, 3); (float)lI rounds at all
    assert (m["pair"] > 2 ** 24) == (F == 33) and m["pair_lo"] > 2 ** 24
