"""GPU parity of the lane-pair PLL's chunk loop (sdr_pll.hip pll_run_split, pair_chunk): the main
loop over pairs of 16-step chunks, the odd last chunk on the fast path, and the checked rest of
n % 16 steps, bit for bit against the oracle's orc_fmpll -- NCO output and final state included.

* sdr_fmpll, both PLL configurations (19 kHz and 114 kHz x 0.5), over two blocks (the second starts
  from the state the first left): n with no chunk, one chunk, odd and even chunk counts, every class
  of rest and the workload's own 7350; 1, 3 and 33 channels (one pair; a partly filled wave; a second
  wave that holds one pair beside 31 empty ones); rows 16-byte aligned (the 16-byte loads and stores)
  and offset by one float (the scalar loader).
* chunk redos: the PLL inputs the oracle's pipeline forms from all-128 silence, a pilot 3 Hz off and a
  weak signal on 5 channels. tests/cpp/pll_chunk_proof_driver.cpp decides on the host, with
  pll_math.h, which chunks the fast step cannot prove: the test requires at least one such chunk in
  each PLL configuration before it believes the GPU comparison exercised a redo.
* the persistent launch: 5 channels x 3 blocks in the dispatch, persistent and fill-by-parts schedules
  (tests/test_gpu_modes.py's runner), mode 0 (trigArg table) and mode 1 (13230 samples: no table).

Reference: pll.cpp:4-61, stereo.cpp:69-114, rds.cpp:95-133."""
from __future__ import annotations

import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FS = 240000.0
CONFIGS = {"stereo19k": (19e3, 2.0, 0.01), "rds114k": (114e3, 0.5, 0.001)}   # stereo.cpp:77, rds.cpp:119
NS = (6, 15, 16, 17, 31, 32, 33, 47, 48, 49, 7350)
CHANNELS = (1, 3, 33)
NBLK = 2
STATE_FIELDS = ("feedbackI", "feedbackQ", "integrator", "phaseEst", "trigOffset")   # lastCarrier: out[0] of the next block


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _tone(freq: float, nch: int, n: int, blk: int, seed: int) -> np.ndarray:
    """A carrier near the PLL's frequency per channel (own offset, phase and level) with a little
    noise, block blk of a continuous stream."""
    rng = np.random.default_rng(seed * 1000 + blk)
    t = (np.arange(n) + blk * n) / FS
    return np.stack([((0.05 + 0.02 * (c % 5)) * np.cos(2 * np.pi * (freq + 1.5 * (c % 7)) * t + 0.4 * c)
                      + 0.004 * rng.standard_normal(n)).astype(np.float32) for c in range(nch)])


def _fmpll_vs_oracle(torch, pkg, oracle, blocks, freq, nco, bw, aligned: bool) -> list[str]:
    """blocks[b][nch][n] through sdr_fmpll and orc_fmpll, one state chain per channel; every output
    word of every block and the final state compared. Returns the mismatches."""
    nch, n = blocks[0].shape
    d_st = pkg.pll_state_tensor(nch)
    st_ref = [oracle.new_pll_state() for _ in range(nch)]
    out_ref = [np.zeros(n + 1, np.float32) for _ in range(nch)]
    for o in out_ref:
        o[-1] = 1.0
    pitch = (n + 8 + 3) // 4 * 4                     # rows a multiple of 16 bytes apart
    off = 0 if aligned else 1                        # ... and one float past a 16-byte boundary
    bad = []
    for b, x in enumerate(blocks):
        d_buf = torch.zeros(nch, pitch, device="cuda")
        d_x = d_buf[:, off:off + n]
        d_x.copy_(torch.from_numpy(x))
        assert (d_x.data_ptr() % 16 == 0) == aligned
        d_out = torch.zeros(nch, n + 1, device="cuda")
        pkg.fmpll(d_out, d_x, freq, FS, d_st, nco, 0.0, bw)
        out = d_out.cpu().numpy()
        for c in range(nch):
            oracle.fmpll(x[c], freq, FS, out_ref[c], st_ref[c], nco, 0.0, bw)
            if not np.array_equal(_u32(out[c]), _u32(out_ref[c])):
                first = int(np.nonzero(_u32(out[c]) != _u32(out_ref[c]))[0][0])
                bad.append(f"out block {b} ch {c} first at {first}")
    got = pkg.pll_state_from_tensor(d_st)
    for c in range(nch):
        for f in STATE_FIELDS:
            g, r = getattr(got[c], f), getattr(st_ref[c], f)
            if not (g == r or (g != g and r != r)):
                bad.append(f"state ch {c} {f}: {g!r} != {r!r}")
    return bad


@pytest.mark.parametrize("aligned", [True, False], ids=["vec16", "offset1"])
@pytest.mark.parametrize("nch", CHANNELS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_fmpll_chunk_counts_bit_exact(pkg, oracle, torch_cuda, cfg, nch, aligned):
    freq, nco, bw = CONFIGS[cfg]
    bad = []
    for n in NS:
        blocks = [_tone(freq, nch, n, b, seed=n) for b in range(NBLK)]
        bad += [f"n {n}: {m}" for m in _fmpll_vs_oracle(torch_cuda, pkg, oracle, blocks, freq, nco, bw, aligned)]
    assert not bad, f"{cfg} nch {nch}: {len(bad)} mismatches, first: {bad[:8]}"


# ---------------------------------------------------------------- chunk redos
REDO_KINDS = ("silence", "pilot_offset", "weak", "silence", "pilot_offset")   # tests/test_gpu_width.py's hostile kinds
REDO_BLOCKS = 2


@pytest.fixture(scope="module")
def proof_driver(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ (the host libraries are built with it)"
    exe = tmp_path_factory.mktemp("pll_proof") / "pll_chunk_proof"
    subprocess.run([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "real-time-sdr_amd" / "csrc"),
                    str(ROOT / "tests" / "cpp" / "pll_chunk_proof_driver.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def hostile_pll_inputs(pkg, synth, oracle, torch_cuda):
    """The two PLLs' inputs (stereo.cpp:74 pilot, rds.cpp:116 squared RDS band) that the oracle's
    pipeline forms from the hostile bytes, [config][block][channel][n]; computed once."""
    torch = torch_cuda
    sys.path.insert(0, str(ROOT))
    import bench
    dev = torch.device("cuda", 0)
    nch = len(REDO_KINDS)
    iq = bench.make_input(torch, nch, REDO_BLOCKS, first_channel=0, device=dev, kinds=list(REDO_KINDS), seed=5)
    host = iq.cpu().numpy()
    x = {"stereo19k": [[None] * nch for _ in range(REDO_BLOCKS)], "rds114k": [[None] * nch for _ in range(REDO_BLOCKS)]}
    for c in range(nch):
        ref = oracle.run_channel(np.ascontiguousarray(host[:, c]), 0, True, intermediates_at=tuple(range(REDO_BLOCKS)))
        for b in range(REDO_BLOCKS):
            x["stereo19k"][b][c] = ref["intermediates"][b]["pilot"].copy()
            x["rds114k"][b][c] = ref["intermediates"][b]["gen_pilot"].copy()
    return {k: [np.stack(rows) for rows in v] for k, v in x.items()}


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_fmpll_chunk_redos_bit_exact(pkg, oracle, torch_cuda, proof_driver, hostile_pll_inputs, cfg):
    freq, nco, bw = CONFIGS[cfg]
    blocks = hostile_pll_inputs[cfg]
    nch, n = blocks[0].shape
    # the first block starts from the reset state, as the driver does
    failed = {}
    for c in range(nch):
        r = subprocess.run([str(proof_driver), repr(freq), repr(FS), repr(bw), str(n)], input=blocks[0][c].tobytes(),
                           capture_output=True, check=True, timeout=60)
        chunks, nbad = (int(v) for v in r.stdout.split())
        assert chunks == n // 16
        failed[f"{REDO_KINDS[c]} ch{c}"] = nbad
    print(f"{cfg}: chunks of block 0 the fast step cannot prove, of {n // 16}: {failed}")
    assert any(v > 0 for v in failed.values()), f"{cfg}: no chunk redo in these inputs ({failed}): choose another seed"
    bad = _fmpll_vs_oracle(torch_cuda, pkg, oracle, blocks, freq, nco, bw, aligned=True)
    assert not bad, f"{cfg}: {len(bad)} mismatches, first: {bad[:8]}"


# ---------------------------------------------------------------- the persistent launch
PERSIST_KINDS = ("normal", "silence", "noise", "pilot_offset", "weak")
PERSIST_BLOCKS = 3
PERSIST_TAB = {0: 1, 1: 0}        # block_if 7350 doubles fit the 64 KiB table, 13230 do not


@pytest.fixture(scope="module", params=[0, 1], ids=["mode0", "mode1"])
def persistent_runs(request, pkg, synth, oracle, torch_cuda):
    """The three schedules of one mode on the same 5 x 3 input, and the oracle's outputs, once."""
    import test_gpu_modes as tm
    torch = torch_cuda
    sys.path.insert(0, str(ROOT))
    import bench
    mode = request.param
    dev = torch.device("cuda", 0)
    gpu = (torch, bench, dev)
    nch = len(PERSIST_KINDS)
    probe = pkg.Pipeline(nch, mode=mode, rds_on=True, device=0)
    info = probe.info
    n_cu = tm._fit_cus(probe)
    plan = probe.plls_plan(n_cu)
    probe.close()
    assert plan["wg_waves"] == 1 and not plan["staged"] and plan["tab_ok"] == PERSIST_TAB[mode], plan
    iq = tm._make_input(torch, synth, info, nch, PERSIST_BLOCKS, dev, list(PERSIST_KINDS), seed=41 + mode)
    host_iq = iq.cpu().numpy()
    runs = {sch: tm._run_schedule(gpu, pkg, iq, mode, sch, n_cu, plan) for sch in tm.SCHEDULES}
    ref = [oracle.run_channel(np.ascontiguousarray(host_iq[:, c]), mode, True) for c in range(nch)]
    return mode, runs, ref, tm


@pytest.mark.parametrize("schedule", ("dispatch", "persistent", "persistent_parts"))
def test_persistent_schedules_bit_exact(persistent_runs, schedule):
    mode, runs, ref, tm = persistent_runs
    got = runs[schedule]
    if got is None:
        pytest.skip("no CU-masked streams: the bench does not run the persistent PLL without them")
    bad = []
    for c in range(len(PERSIST_KINDS)):
        for b in range(PERSIST_BLOCKS):
            tm._compare(got, b, c, ref[c], f"{PERSIST_KINDS[c]} ch{c} b{b}", bad)
    assert not bad, f"mode {mode} {schedule}: {len(bad)} mismatches, first: {bad[:10]}"
