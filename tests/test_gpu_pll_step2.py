"""GPU parity of the lane-pair PLL's fast chunk without its per-step |e| range test (sdr_pll.hip
pll_step_split, pair_chunk; pll_math.h "The cut at +-pi"), bit for bit against the oracle.

* the cut itself: sdr_fmpll from states whose previous trigArg sits on and next to k pi/2, |k| <= 8
  (feedback RN32(cos t), RN32(sin t) of that t, so the fast chunk runs from the first step), with
  inputs of either sign: the first phase-detector result is within 2^-22 of +pi or -pi. NCO output
  (the phases) and end state, both PLL configurations, three chunks and a rest of 6 steps.
* 5 channels x 3 blocks of mode 0 -- all-128 silence (atan2(+-0, +-0)), random bytes (e anywhere in
  [-pi, pi], next to +-pi included), a pilot 3 Hz off (phaseEst drifts without bound), a normal and a
  weak station -- in the dispatch and the persistent schedule: every stereo and RDS output of the
  pipeline (tests/test_gpu_modes.py's runner and comparison); and the two PLLs' own inputs of those
  channels (the oracle's intermediates) through sdr_fmpll: phases and state.
* the same step without the trigArg table (TAB = false): channels sharing a trigOffset just below the
  table bound of the 114 kHz PLL and just across it (tests/test_gpu_primitives.py
  test_fmpll_long_stream_shared_offset's set-up at n = 54: three chunks and the rest).

Reference: pll.cpp:4-61, stereo.cpp:69-114, rds.cpp:95-167."""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FS = 240000.0
CONFIGS = {"stereo19k": (19e3, 2.0, 0.01), "rds114k": (114e3, 0.5, 0.001)}   # stereo.cpp:77, rds.cpp:119
KINDS = ("silence", "noise", "pilot_offset", "normal", "weak")
NBLOCKS = 3
N_SHORT = 54                       # 3 chunks of 16 (the loop's pair and the odd last chunk) + 6 checked steps
STATE_FIELDS = ("feedbackI", "feedbackQ", "integrator", "phaseEst", "trigOffset", "lastCarrier")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run_states(torch, pkg, oracle, states, x, freq, nco, bw) -> list[str]:
    """One sdr_fmpll call on x[nch][n] from the given states (fbI, fbQ, integ, ph, toff, lastCarrier)
    against orc_fmpll per channel: outputs and end states."""
    nch, n = x.shape
    arr = (pkg.PllState * nch)()
    refs = []
    for i, s in enumerate(states):
        arr[i] = pkg.PllState(*s)
        refs.append(oracle.PllState(*s))
    d_st = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).cuda()
    d_out = torch.zeros(nch, n + 1, device="cuda")
    pkg.fmpll(d_out, torch.from_numpy(x).cuda(), freq, FS, d_st, nco, 0.0, bw)
    out = d_out.cpu().numpy()
    got = pkg.pll_state_from_tensor(d_st)
    bad = []
    for c in range(nch):
        o = np.zeros(n + 1, np.float32)
        o[-1] = 1.0
        oracle.fmpll(x[c], freq, FS, o, refs[c], nco, 0.0, bw)
        if not np.array_equal(_u32(out[c]), _u32(o)):
            bad.append(f"ch {c} out first at {int(np.nonzero(_u32(out[c]) != _u32(o))[0][0])}")
        for f in STATE_FIELDS:
            g, r = getattr(got[c], f), getattr(refs[c], f)
            if not (g == r or (g != g and r != r)):
                bad.append(f"ch {c} {f}: {g!r} != {r!r}")
    return bad


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_fmpll_at_the_cut_bit_exact(pkg, oracle, torch_cuda, cfg):
    freq, nco, bw = CONFIGS[cfg]
    states, rows = [], []
    rng = np.random.default_rng(15)
    for k in range(-8, 9):
        for du in (-1, 0, 1):
            for sign in (1.0, -1.0):
                ph = np.float32(k * (np.pi / 2))
                if du:
                    ph = np.nextafter(ph, np.float32(np.inf * du), dtype=np.float32)
                # trigOffset 0: the previous trigArg is phaseEst itself (pll.cpp:47)
                fI, fQ = np.float32(np.cos(np.float64(ph))), np.float32(np.sin(np.float64(ph)))
                states.append((float(fI), float(fQ), 1e-5, float(ph), 0.0, 1.0))
                rows.append((sign * (0.05 + 0.01 * rng.random(N_SHORT))).astype(np.float32))
    bad = _run_states(torch_cuda, pkg, oracle, states, np.stack(rows), freq, nco, bw)
    assert not bad, f"{cfg}: {len(bad)} mismatches, first: {bad[:8]}"


def test_fmpll_without_table_bit_exact(pkg, oracle, torch_cuda):
    freq, nco, bw = CONFIGS["rds114k"]
    w = 2 * np.pi * np.float32(freq / FS)
    bound = 1.375 * 2.0 ** 29                             # PLL_TAB_WT_MAX
    n, nch = N_SHORT, 6
    rng = np.random.default_rng(16)
    t = np.arange(n) / FS
    x = np.stack([(0.05 * np.cos(2 * np.pi * freq * t + 0.1 * c) + 0.02 * rng.standard_normal(n)).astype(np.float32)
                  for c in range(nch)])
    # the launch keeps the table while |w| (trigOffset + n + 1) stays below the bound
    for toff in (float(int(bound / w) - n - 2), float(int(bound / w) - n // 2)):
        states = [(1.0, 0.0, 0.0, 0.0, toff, 1.0)] * nch
        bad = _run_states(torch_cuda, pkg, oracle, states, x, freq, nco, bw)
        assert not bad, f"trigOffset {toff:g}: {len(bad)} mismatches, first: {bad[:8]}"


@pytest.fixture(scope="module")
def mode0_runs(pkg, synth, oracle, torch_cuda):
    """The dispatch and the persistent schedule of mode 0 on one 5 x 3 input, and the oracle's outputs
    and PLL inputs of the same bytes, once."""
    import test_gpu_modes as tm
    torch = torch_cuda
    sys.path.insert(0, str(ROOT))
    import bench
    dev = torch.device("cuda", 0)
    gpu = (torch, bench, dev)
    nch = len(KINDS)
    probe = pkg.Pipeline(nch, mode=0, rds_on=True, device=0)
    info = probe.info
    n_cu = tm._fit_cus(probe)
    plan = probe.plls_plan(n_cu)
    probe.close()
    assert plan["wg_waves"] == 1 and not plan["staged"] and plan["tab_ok"] == 1, plan
    iq = tm._make_input(torch, synth, info, nch, NBLOCKS, dev, list(KINDS), seed=152)
    host_iq = iq.cpu().numpy()
    runs = {sch: tm._run_schedule(gpu, pkg, iq, 0, sch, n_cu, plan) for sch in ("dispatch", "persistent")}
    ref = [oracle.run_channel(np.ascontiguousarray(host_iq[:, c]), 0, True, intermediates_at=tuple(range(NBLOCKS)))
           for c in range(nch)]
    return runs, ref, tm


@pytest.mark.parametrize("schedule", ("dispatch", "persistent"))
def test_mode0_schedules_bit_exact(mode0_runs, schedule):
    runs, ref, tm = mode0_runs
    got = runs[schedule]
    if got is None:
        pytest.skip("no CU-masked streams: the bench does not run the persistent PLL without them")
    bad = []
    for c in range(len(KINDS)):
        for b in range(NBLOCKS):
            tm._compare(got, b, c, ref[c], f"{KINDS[c]} ch{c} b{b}", bad)
    assert not bad, f"{schedule}: {len(bad)} mismatches, first: {bad[:10]}"


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_mode0_pll_inputs_phases_and_state(pkg, oracle, torch_cuda, mode0_runs, cfg):
    import test_gpu_pll_chunk as tc
    _, ref, _ = mode0_runs
    key = {"stereo19k": "pilot", "rds114k": "gen_pilot"}[cfg]        # stereo.cpp:74, rds.cpp:116
    blocks = [np.stack([ref[c]["intermediates"][b][key] for c in range(len(KINDS))]) for b in range(NBLOCKS)]
    freq, nco, bw = CONFIGS[cfg]
    bad = tc._fmpll_vs_oracle(torch_cuda, pkg, oracle, blocks, freq, nco, bw, aligned=True)
    assert not bad, f"{cfg}: {len(bad)} mismatches, first: {bad[:8]}"
