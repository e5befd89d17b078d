"""GPU parity of the lane-pair PLL's phase stores (sdr_pll.hip pll_run_split, store_chunk): with 16-byte
rows the even lane of a pair stores phases i0 .. i0+7 of a 16-step chunk and the odd lane i0+8 .. i0+15,
two stores per chunk and lane; the rest loop and rows that are not 16-byte aligned store phase by phase.

sdr_fmpll against the oracle's orc_fmpll, bit for bit -- every row of the NCO output (word i+1 is the
cosine of phase i, so a phase stored in the wrong place shows at its own sample) and the final state --
over two consecutive calls, the second from the state the first stored:

* both PLL configurations (19 kHz and 114 kHz at 240 kHz);
* the smallest block lengths that reach every store path: 6 (rest only), 16 (one chunk: the call after
  the loop), 22 (that chunk plus a rest), 38 (one pair of loop chunks plus a rest), 54 (a pair, the odd
  chunk and a rest), 70 (two pairs and a rest);
* 3 channels (a half-filled wave, an odd pair count) and 33 (two waves);
* rows, rotating with the block length so that every kind meets every count of channels: a clean tone, a
  tone 3 Hz off, all zeros, and uniform noise -- its chunks fail their proofs, so what is stored is a
  redone chunk's phases (tests/cpp/pll_chunk_proof_driver.cpp, the host's copy of the proof, confirms
  that such chunks exist);
* one case reads x from an element offset of 1 (rows not 16-byte aligned: the scalar stores); its output
  must equal the aligned case's.

Every chunk is compared half by half, so a mismatch names the pair's lane whose store it was and the
sample; a check without a GPU swaps two halves of the oracle's own output and requires exactly that report.
The oracle's runs over these inputs are finite and repeat bit for bit (also checked without a GPU).

Reference: pll.cpp:4-61."""
from __future__ import annotations

import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FS = 240000.0
CONFIGS = {"stereo19k": (19e3, 2.0, 0.01), "rds114k": (114e3, 0.5, 0.001)}   # stereo.cpp:77, rds.cpp:119
NS = (6, 16, 22, 38, 54, 70)
CHANNELS = (3, 33)
NCALLS = 2
CHUNK = 16
KINDS = ("tone", "tone_off", "zeros", "noise")
STATE_FIELDS = ("feedbackI", "feedbackQ", "integrator", "phaseEst", "trigOffset")   # lastCarrier: out[0] of the next call


def _kind(n: int, c: int) -> str:
    return KINDS[(c + NS.index(n)) % len(KINDS)]


def _rows(freq: float, nch: int, n: int, call: int) -> np.ndarray:
    """Call `call` of a continuous stream per channel."""
    t = (np.arange(n) + call * n) / FS
    rows = []
    for c in range(nch):
        kind = _kind(n, c)
        if kind == "tone":
            x = 0.06 * np.cos(2 * np.pi * freq * t + 0.4 * c)
        elif kind == "tone_off":
            x = 0.05 * np.cos(2 * np.pi * (freq + 3.0) * t + 0.3 * c)
        elif kind == "zeros":
            x = np.zeros(n)
        else:
            x = np.random.default_rng(1000 * n + 10 * c + call).uniform(-0.5, 0.5, n)
        rows.append(x.astype(np.float32))
    return np.stack(rows)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _oracle_case(oracle, cfg: str, nch: int, n: int):
    """(inputs per call [nch][n], the oracle's out rows per call [nch][n + 1], its final states)"""
    freq, nco, bw = CONFIGS[cfg]
    xs = [_rows(freq, nch, n, k) for k in range(NCALLS)]
    st = [oracle.new_pll_state() for _ in range(nch)]
    out = [np.zeros(n + 1, np.float32) for _ in range(nch)]
    for o in out:
        o[-1] = 1.0
    outs = []
    for x in xs:
        for c in range(nch):
            oracle.fmpll(x[c], freq, FS, out[c], st[c], nco, 0.0, bw)
        outs.append(np.stack(out))
    return xs, outs, st


@pytest.fixture(scope="module")
def reference(oracle):
    """The oracle over every case, once; the tests only read it."""
    ref = {(cfg, nch, n): _oracle_case(oracle, cfg, nch, n) for cfg in CONFIGS for nch in CHANNELS for n in NS}
    for key, (_, outs, st) in ref.items():
        assert all(np.isfinite(o).all() for o in outs), key
        assert all(np.isfinite(getattr(s, f)) for s in st for f in STATE_FIELDS), key
    return ref


def _compare_rows(got: np.ndarray, want: np.ndarray, where: str) -> list[str]:
    """One call's out rows [nch][n + 1]: word 0 (the carried sample), every chunk's two stored halves
    apart (word 1 + i belongs to phase i), and the rest. Each mismatch names the first differing sample."""
    nch, n1 = want.shape
    n = n1 - 1
    nchunks = n // CHUNK
    g, w = _u32(got), _u32(want)
    bad = []

    def piece(c, lo, hi, what):   # phases [lo, hi)
        d = np.nonzero(g[c, 1 + lo:1 + hi] != w[c, 1 + lo:1 + hi])[0]
        if d.size:
            bad.append(f"{where} ch {c} {what}: first at sample {lo + int(d[0])}")

    for c in range(nch):
        if g[c, 0] != w[c, 0]:
            bad.append(f"{where} ch {c} out[0]")
        for q in range(nchunks):
            piece(c, q * CHUNK, q * CHUNK + CHUNK // 2, f"chunk {q} first half (the even lane's store)")
            piece(c, q * CHUNK + CHUNK // 2, (q + 1) * CHUNK, f"chunk {q} second half (the odd lane's store)")
        piece(c, nchunks * CHUNK, n, "rest")
    return bad


def _compare_state(got, want, where: str) -> list[str]:
    bad = []
    for c, (a, b) in enumerate(zip(got, want)):
        for f in STATE_FIELDS:
            x, y = getattr(a, f), getattr(b, f)
            if np.array(x).tobytes() != np.array(y).tobytes():
                bad.append(f"{where} state ch {c} {f}: {x!r} != {y!r}")
    return bad


def _gpu_case(torch, pkg, cfg: str, xs, aligned: bool):
    """sdr_fmpll over the calls, one state chain per channel: out rows per call and the final states."""
    freq, nco, bw = CONFIGS[cfg]
    nch, n = xs[0].shape
    d_st = pkg.pll_state_tensor(nch)
    pitch = (n + 8 + 3) // 4 * 4                     # rows a multiple of 16 bytes apart
    off = 0 if aligned else 1                        # ... or one float past a 16-byte boundary
    outs = []
    d_out = torch.zeros(nch, n + 1, device="cuda")
    d_out[:, -1] = 1.0
    for x in xs:
        d_buf = torch.zeros(nch, pitch, device="cuda")
        d_x = d_buf[:, off:off + n]
        d_x.copy_(torch.from_numpy(x))
        assert (d_x.data_ptr() % 16 == 0) == aligned
        pkg.fmpll(d_out, d_x, freq, FS, d_st, nco, 0.0, bw)
        outs.append(d_out.cpu().numpy())
    return outs, pkg.pll_state_from_tensor(d_st)


# ---------------------------------------------------------------- without a GPU
def test_oracle_runs_finite_and_deterministic(oracle, reference):
    for cfg in CONFIGS:
        for n in NS:
            _, outs, st = reference[(cfg, 3, n)]
            _, outs2, st2 = _oracle_case(oracle, cfg, 3, n)
            for a, b in zip(outs, outs2):
                assert np.array_equal(_u32(a), _u32(b)), (cfg, n)
            assert not _compare_state(st2, st, f"{cfg} n {n}")


def test_comparer_names_swapped_halves(reference):
    _, outs, _ = reference[("stereo19k", 3, 54)]
    want = outs[1]
    got = want.copy()
    # chunk 2 of channel 0 (a clean tone at n = 54: no two phases alike): the two halves exchanged
    got[0, 1 + 32:1 + 40], got[0, 1 + 40:1 + 48] = want[0, 1 + 40:1 + 48].copy(), want[0, 1 + 32:1 + 40].copy()
    assert _kind(54, 0) == "tone"
    bad = _compare_rows(got, want, "call 1")
    assert bad == ["call 1 ch 0 chunk 2 first half (the even lane's store): first at sample 32",
                   "call 1 ch 0 chunk 2 second half (the odd lane's store): first at sample 40"], bad
    assert not _compare_rows(want, want, "call 1")


# ---------------------------------------------------------------- on the GPU
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.gpu
@pytest.mark.parametrize("nch", CHANNELS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_fmpll_phase_stores_bit_exact(pkg, reference, torch_cuda, cfg, nch):
    bad = []
    for n in NS:
        xs, want, st = reference[(cfg, nch, n)]
        got, got_st = _gpu_case(torch_cuda, pkg, cfg, xs, aligned=True)
        for k in range(NCALLS):
            bad += _compare_rows(got[k], want[k], f"n {n} call {k}")
        bad += _compare_state(got_st, st, f"n {n}")
    assert not bad, f"{cfg} nch {nch}: {len(bad)} mismatches, first: {bad[:8]}"


@pytest.mark.gpu
def test_fmpll_unaligned_rows_equal_aligned(pkg, reference, torch_cuda):
    cfg, nch = "stereo19k", 3
    bad = []
    for n in NS:
        xs, want, st = reference[(cfg, nch, n)]
        got, got_st = _gpu_case(torch_cuda, pkg, cfg, xs, aligned=False)
        ali, ali_st = _gpu_case(torch_cuda, pkg, cfg, xs, aligned=True)
        for k in range(NCALLS):
            bad += _compare_rows(got[k], ali[k], f"n {n} call {k} offset against aligned")
            bad += _compare_rows(got[k], want[k], f"n {n} call {k} offset against the oracle")
        bad += _compare_state(got_st, ali_st, f"n {n} offset against aligned")
        bad += _compare_state(got_st, st, f"n {n} offset against the oracle")
    assert not bad, f"{len(bad)} mismatches, first: {bad[:8]}"


# ---------------------------------------------------------------- without a GPU: the noise rows are redone
@pytest.fixture(scope="module")
def proof_driver(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ (the host libraries are built with it)"
    exe = tmp_path_factory.mktemp("pll_proof") / "pll_chunk_proof"
    subprocess.run([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "real-time-sdr_amd" / "csrc"),
                    str(ROOT / "tests" / "cpp" / "pll_chunk_proof_driver.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_noise_rows_store_redone_chunks(reference, proof_driver, cfg):
    """The host's copy of the proof over the noise rows' first call (from the reset state, as the driver
    starts): at every block length with a chunk, some chunk of a noise row cannot be proven, so the GPU
    comparison above covered the store of a redone chunk in the after-loop call and in the loop."""
    freq, _, bw = CONFIGS[cfg]
    for n in NS:
        if n < CHUNK:
            continue
        xs, _, _ = reference[(cfg, 33, n)]
        nbad = 0
        for c in range(33):
            if _kind(n, c) != "noise":
                continue
            r = subprocess.run([str(proof_driver), repr(freq), repr(FS), repr(bw), str(n)], input=xs[0][c].tobytes(),
                               capture_output=True, check=True, timeout=60)
            chunks, failed = (int(v) for v in r.stdout.split())
            assert chunks == n // CHUNK
            nbad += failed
        assert nbad > 0, f"{cfg} n {n}: every chunk of the noise rows is proven: choose other noise"
