"""GPU parity of the lane-pair PLL with one loop-filter state word per lane (sdr_pll.hip
pll_step_split: the even lane of a pair owns phaseEst, the odd lane the integrator).

5 channels -- an odd count, so the last lane pairs of each PLL's wave are empty and the wave runs
partly filled -- over 3 blocks through `Pipeline` in the bench's split-stage schedule, with one
sdr_plls dispatch per block (`dispatch`: k_pll) and with one persistent launch for all blocks
(`persistent`: k_pll_multi). One channel each of normal, silence (atan2(+-0, +-0): e = +-0 on every
step), random bytes (unlocked, frequent chunk redos through the checked step and back), a pilot 3 Hz
off (phaseEst drifts) and a weak signal. fm_demod, mono, stereo and rds_clean of every channel and
block are compared bit for bit with the oracle on the same bytes: blocks 1 and 2 start from the state
each lane's word left behind (split_to_full at a block's end, full_to_split at the next one's start).

Reference: pll.cpp:34-53, stereo.cpp:69-114, rds.cpp:95-133."""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

KINDS = ("normal", "silence", "noise", "pilot_offset", "weak")
NCH = len(KINDS)
NBLOCKS = 3
SCHEDULES = ("dispatch", "persistent")


def _run(torch, pkg, bench, iq, dev, schedule: str) -> dict:
    """bench.GpuStepper.step's stream schedule on a fresh context, outputs captured per block."""
    pipe = pkg.Pipeline(NCH, mode=0, rds_on=True, device=0)
    info = pipe.info
    created: list[int] = []
    persistent = schedule == "persistent"
    try:
        s_fe, s_pll, s_post, _ = bench.cu_masked_streams(torch, pkg, dev, "64", created)
    except (RuntimeError, AttributeError):
        if persistent:
            pipe.close()
            pytest.skip("no CU-masked streams: the persistent PLL is not run without them")
        s_fe, s_pll, s_post = (torch.cuda.Stream(dev) for _ in range(3))
    ev = lambda: [torch.cuda.Event() for _ in range(NBLOCKS)]  # noqa: E731
    pre_done, pll_done, post_done = ev(), ev(), ev()
    cap = {"fm": torch.empty(NBLOCKS, NCH, info.block_if, dtype=torch.float32, device=dev),
           "mono": torch.empty(NBLOCKS, NCH, info.n_audio, dtype=torch.int16, device=dev),
           "lr": torch.empty(NBLOCKS, NCH, 2 * info.n_audio, dtype=torch.int16, device=dev),
           "clean": torch.empty(NBLOCKS, NCH, info.n_rds, dtype=torch.float32, device=dev)}
    if persistent:
        pipe.plls_launch(NBLOCKS, stream=s_pll)
    for b in range(NBLOCKS):
        if b >= 2:
            s_fe.wait_event(post_done[b - 2])
        pipe.frontend(iq[b], stream=s_fe)
        pipe.fm_demod(cap["fm"][b], stream=s_fe)
        pipe.mono(cap["mono"][b], stream=s_fe)
        pipe.pre(stream=s_fe)
        if persistent:
            pipe.plls_signal(stream=s_fe)
            pipe.plls_wait(stream=s_post)
        else:
            pre_done[b].record(s_fe)
            s_pll.wait_event(pre_done[b])
            pipe.plls(stream=s_pll)
            pll_done[b].record(s_pll)
            s_post.wait_event(pll_done[b])
        pipe.stereo_post(cap["lr"][b], stream=s_post)
        pipe.rds_post(cap["clean"][b], bits=False, stream=s_post)
        post_done[b].record(s_post)
    torch.cuda.synchronize(dev)
    if persistent:
        assert len(pipe.plls_report(stream=s_pll)) == NBLOCKS   # raises if a block's wait timed out
    host = {k: v.cpu().numpy() for k, v in cap.items()}
    pipe.close()
    bench.destroy_masked_streams(torch, pkg, dev, created)
    return host


@pytest.fixture(scope="module")
def pair_case(pkg, synth):
    """The input bytes (generated on the device, copied back) and the oracle's outputs, once."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, str(ROOT))
    import bench
    import oracle
    dev = torch.device("cuda", 0)
    iq = bench.make_input(torch, NCH, NBLOCKS, first_channel=0, device=dev, kinds=list(KINDS), seed=11)
    host_iq = iq.cpu().numpy()
    ref = [oracle.run_channel(np.ascontiguousarray(host_iq[:, c]), 0, True) for c in range(NCH)]
    return torch, bench, dev, iq, ref


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_pair_pll_odd_channel_count_bit_exact(pkg, pair_case, schedule):
    torch, bench, dev, iq, ref = pair_case
    got = _run(torch, pkg, bench, iq, dev, schedule)
    bad = []
    for c in range(NCH):
        for b in range(NBLOCKS):
            where = f"{KINDS[c]} ch{c} b{b}"
            if not np.array_equal(got["fm"][b, c].view(np.uint32), ref[c]["fm_demod"][b].view(np.uint32)):
                bad.append(f"fm_demod {where}")
            if not np.array_equal(got["mono"][b, c], ref[c]["mono"][b]):
                bad.append(f"mono {where}")
            if not np.array_equal(got["lr"][b, c], ref[c]["stereo"][b]):
                bad.append(f"stereo {where}")
            if not np.array_equal(got["clean"][b, c].view(np.uint32), ref[c]["rds_clean"][b].view(np.uint32)):
                bad.append(f"rds_clean {where}")
    assert not bad, f"{schedule}: {len(bad)} mismatches, first: {bad[:10]}"
