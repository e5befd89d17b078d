"""GPU, world_size 1: bench.py's timed phase as the driver runs it (bench.run_rank with the real
GpuStepper), at a small width: the persistent PLL launch per phase, the first block's front end and
pre-PLL FIRs and the last block's post stage on the all-CU stream, mono after the PLL signal. Every
block's captured mono, stereo and RDS bits of the sampled channels bit-exact against the oracle
(bench.verify_captured), and the timeline the bench reports (fill, drain, PLL span) present.
Reference: project.cpp:134-136, rffrontend.cpp:58-71, mono.cpp:34-42, stereo.cpp:77-107,
rds.cpp:105-167."""
from __future__ import annotations

import argparse
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(300)
def test_bench_phase_edges_world1(monkeypatch):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, str(ROOT))
    import bench
    monkeypatch.setenv("SDR_BENCH_CPU_CORES", "4")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = argparse.Namespace(channels=48, warmup=3, steps=5, full=True, no_gather=True, no_isolated=True,
                              no_cpu_baseline=False, cpu_timing=False, numerics="exact", gpus=1, backend="nccl")
    res = bench.run_rank(args, 1, 0, 0)
    assert res["verified"] is True, res.get("cpu_baseline", {}).get("verified")
    pll = res["pll"]
    assert pll["mode"] == "persistent", pll["mode"]
    tl = pll["timeline"]
    assert tl["fill_ms"] > 0 and tl["drain_ms"] > 0 and tl["pll_span_ms"] > 0, tl
    assert res["steps"] == 5 and res["n_gpus"] == 1


@pytest.mark.timeout(300)
@pytest.mark.parametrize("ring", [None, 7], ids=["plain", "full_input_wraps"])
def test_bench_dump_outputs_last_step(monkeypatch, tmp_path, oracle, ring):
    """A plain run (no --full) with --dump-outputs: the result line without the checker's legs, and
    DIR/<name>.npy holding the last timed step's outputs, one float32 row per channel. The bench's
    input is seeded, so the same rows come out of the oracle run on the regenerated input: mono,
    stereo and rds_clean of the last block bit for bit, the RDS bits up to rds_nbits and -1 after.
    full_input_wraps: a run of more blocks than bench.INPUT_RING holds (here 7) reads them round,
    block b being block b % 7; the same dump check on that sequence, and with --full every block of
    the checked channels against the oracle and the queue-plumbed receiver on the blocks before the
    wrap."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, str(ROOT))
    import bench
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("SDR_BENCH_CPU_CORES", "4")
    if ring:
        monkeypatch.setattr(bench, "INPUT_RING", ring)
    nch, warmup, steps = 48, 3, 6      # RDS decodes from block 6 on; the last block is 8
    out = tmp_path / "dump"
    args = argparse.Namespace(channels=nch, warmup=warmup, steps=steps, full=bool(ring), dump_outputs=str(out),
                              no_gather=True, no_isolated=not ring, no_cpu_baseline=False, cpu_timing=False,
                              numerics="exact", gpus=1, backend="nccl")
    res = bench.run_rank(args, 1, 0, 0)
    assert res["steps"] == steps and res["ms_per_step"] > 0
    if ring:
        assert res["verified"] is True, res["cpu_baseline"].get("verified")
        assert res["cpu_baseline"]["verified"]["blocks"] == warmup + steps
        qp = res["queue_plumbed"]
        assert qp.get("outputs_equal_to_bench_capture") is True and qp["timed_run_outputs_equal"] is True, qp
        assert f"({ring} blocks" in qp["input"]
    else:
        assert res["verified"] is None
        assert res["cpu_baseline"] is None and "frontend_isolated" not in res and "queue_plumbed" not in res
    got = {p.stem: np.load(p) for p in out.iterdir()}
    assert sorted(got) == ["mono", "rds_bits", "rds_clean", "rds_nbits", "stereo"]
    assert all(a.dtype == np.float32 and a.shape[0] == nch for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64e6
    last = warmup + steps - 1
    iq = bench.make_input(torch, nch, ring or last + 1, first_channel=0, device=torch.device("cuda", 0))
    iq = iq[torch.arange(last + 1, device=iq.device) % iq.shape[0]]
    decoded = 0
    for c in (0, 17, nch - 1):
        ref = oracle.run_channel(np.ascontiguousarray(iq[:, c].cpu().numpy()), 0, True)
        assert np.array_equal(got["mono"][c], ref["mono"][last].astype(np.float32)), f"mono ch {c}"
        assert np.array_equal(got["stereo"][c], ref["stereo"][last].astype(np.float32)), f"stereo ch {c}"
        assert np.array_equal(got["rds_clean"][c].view(np.uint32), ref["rds_clean"][last].view(np.uint32)), f"rds ch {c}"
        rb = ref["bits"][last]
        n = int(got["rds_nbits"][c])
        assert n == (-1 if rb is None else len(rb)), f"nbits ch {c}"
        assert np.array_equal(got["rds_bits"][c, :max(n, 0)], np.asarray([] if rb is None else rb, np.float32))
        assert (got["rds_bits"][c, max(n, 0):] == -1).all()
        decoded += rb is not None
    assert decoded or ring, "no checked channel decoded RDS bits in the last block"
