"""GPU parity of modes 1-3 (project.cpp:76-103) in the bench's schedules, on inputs generated at the
mode's own sample rate (synth.TorchMultiplexBatch(fs = rf_Fs): a 19 kHz pilot the PLLs lock to,
tests/test_synth_rates.py), bit for bit against the oracle on the same bytes.

The trigArg table of the PLL kernels holds block_if doubles and exists only while it fits 64 KiB
(sdr_pll.hip pll_tab): modes 1 and 3 (13230 and 12800 samples) run the TAB = false instantiations of
every PLL kernel from reset, the ones mode 0 enters once |w| (trigOffset + n + 1) passes
PLL_TAB_WT_MAX, about 17 minutes into a reception. These tests are the ones that reach them in the
persistent launch k_pll_multi: one-wave groups (the lane-pair chunk and its gated fill variant),
four-wave groups with the register prefetch (pll_run_split, the fill block) and with the LDS-staged
loop (pll_run_split_coal), and the engine's two single-PLL launches (sdr_multi --mode). Mode 2 (8000
samples) keeps the table, beside the staged loop's ring. Each test asserts the launch's plan
(Pipeline.plls_plan) before it launches, so it fails when its shape stops reaching the kernel it
names.

Reference: rffrontend.cpp:58-71, demod.cpp:8-19, pll.cpp:34-53, mono.cpp:22-60, stereo.cpp:69-114,
rds.cpp:95-167."""
from __future__ import annotations

import concurrent.futures as cf
import multiprocessing as mp
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

MODES = (1, 2, 3)
TAB_OK = {1: 0, 2: 1, 3: 0}       # block_if 13230, 8000, 12800 doubles against 64 KiB
FIRST_DECODE = 6                  # rds.cpp:135: blocks 0-5 do not decode
KEYS = ("fm", "mono", "lr", "clean", "offset", "nsym", "symbols", "nbits", "bits")

# a: 67 channels = three PLL waves per job, the last with 3 channels and an empty lane pair beside them;
# channels 63 / 64 straddle the exact front end's wave boundary; 9 blocks = three decoding blocks
NCH_A, NB_A = 67, 9
SCHEDULES = ("dispatch", "persistent", "persistent_parts")


@pytest.fixture(scope="module")
def gpu(pkg, synth):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, str(ROOT))
    import bench
    return torch, bench, torch.device("cuda", 0)


def _make_input(torch, synth, info, nch, nblocks, dev, kinds, seed, first_channel=0):
    """[nblocks][nch][2*block_iq] u8 on the device, generated there at the mode's rf_Fs; rows padded to
    16 bytes as bench.make_input pads them."""
    row = 2 * info.block_iq
    d = torch.empty((nblocks, nch, (row + 15) // 16 * 16), dtype=torch.uint8, device=dev)[:, :, :row]
    gen = synth.TorchMultiplexBatch(torch, nch, first_channel, dev, kinds=kinds, seed=seed, fs=info.rf_Fs)
    for b in range(nblocks):
        gen.next_block(info.block_iq, out=d[b])
    torch.cuda.synchronize(dev)
    return d


def _compare(d, b, c, ref, where, bad, j=None):
    """Every output of block b of channel c (row j of d's arrays) against the oracle's."""
    j = c if j is None else j
    if not np.array_equal(d["fm"][b, j].view(np.uint32), ref["fm_demod"][b].view(np.uint32)):
        bad.append(f"fm_demod {where}")
    if not np.array_equal(d["mono"][b, j], ref["mono"][b]):
        bad.append(f"mono {where}")
    if not np.array_equal(d["lr"][b, j], ref["stereo"][b]):
        bad.append(f"stereo {where}")
    if not np.array_equal(d["clean"][b, j].view(np.uint32), ref["rds_clean"][b].view(np.uint32)):
        bad.append(f"rds_clean {where}")
    if (ref["bits"][b] is None) != (b < FIRST_DECODE):
        bad.append(f"oracle decode start {where}")
    if ref["bits"][b] is None:
        if int(d["nbits"][b, j]) != -1:
            bad.append(f"nbits {where}")
        return
    if int(d["offset"][b, j]) != int(ref["offset"][b]):
        bad.append(f"offset {where}")
    ns = int(d["nsym"][b, j])
    if ns != len(ref["symbols"][b]) or not np.array_equal(d["symbols"][b, j, :ns], ref["symbols"][b]):
        bad.append(f"symbols {where}")
    nb = int(d["nbits"][b, j])
    if nb != len(ref["bits"][b]) or not np.array_equal(d["bits"][b, j, :nb], ref["bits"][b]):
        bad.append(f"bits {where}")


def _check(args):
    """Worker: the oracle on channels [lo, hi) of the memory-mapped inputs, compared with the GPU
    outputs of every schedule that ran (the oracle runs once per channel)."""
    path, lo, hi, mode, nblocks = args
    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle
    iq = np.load(os.path.join(path, "iq.npy"), mmap_mode="r")
    runs = {sch: {k: np.load(os.path.join(path, f"{sch}_{k}.npy"), mmap_mode="r") for k in KEYS}
            for sch in SCHEDULES if os.path.exists(os.path.join(path, f"{sch}_fm.npy"))}
    bad = {sch: [] for sch in runs}
    for c in range(lo, hi):
        ref = oracle.run_channel(np.ascontiguousarray(iq[:, c]), mode, True)
        for sch, d in runs.items():
            for b in range(nblocks):
                _compare(d, b, c, ref, f"ch{c} b{b}", bad[sch])
    return bad


def _capture_buffers(torch, pkg, info, nblocks, nch, dev):
    u8, i32 = torch.uint8, torch.int32
    return {"fm": torch.empty(nblocks, nch, info.block_if, dtype=torch.float32, device=dev),
            "mono": torch.empty(nblocks, nch, info.n_audio, dtype=torch.int16, device=dev),
            "lr": torch.empty(nblocks, nch, 2 * info.n_audio, dtype=torch.int16, device=dev),
            "clean": torch.empty(nblocks, nch, info.n_rds, dtype=torch.float32, device=dev),
            "offset": torch.empty(nblocks, nch, dtype=i32, device=dev),
            "nsym": torch.empty(nblocks, nch, dtype=i32, device=dev),
            "symbols": torch.empty(nblocks, nch, pkg.SDR_MAX_SYMS, dtype=u8, device=dev),
            "nbits": torch.empty(nblocks, nch, dtype=i32, device=dev),
            "bits": torch.empty(nblocks, nch, pkg.SDR_MAX_BITS, dtype=u8, device=dev)}


def _run_schedule(gpu, pkg, iq, mode: int, schedule: str, n_cu: int, plan: dict):
    """bench.GpuStepper.step's split-stage schedule on a fresh context of `mode`, outputs captured (as
    tests/test_gpu_width.py runs mode 0): front end + pre-PLL FIRs, the PLLs, the post stage, each on
    its own CU-masked stream; the PLLs as one dispatch per block, or as ONE persistent launch (with
    the first block through frontend_pre_parts for persistent_parts). None: no CU-masked streams for a
    persistent schedule."""
    torch, bench, dev = gpu
    nblocks, nch = iq.shape[0], iq.shape[1]
    pipe = pkg.Pipeline(nch, mode=mode, rds_on=True, device=0)
    info = pipe.info
    assert pipe.plls_plan(n_cu) == plan, f"mode {mode}: the PLL launch on {n_cu} CUs takes another kernel"
    persistent = schedule.startswith("persistent")
    created: list[int] = []
    try:
        s_fe, s_pll, s_post, _ = bench.cu_masked_streams(torch, pkg, dev, str(n_cu), created)
    except (RuntimeError, AttributeError):
        if persistent:
            pipe.close()
            return None
        s_fe, s_pll, s_post = (torch.cuda.Stream(dev) for _ in range(3))
    E = lambda: torch.cuda.Event()  # noqa: E731
    pre_done, pll_done, post_done = ([E() for _ in range(nblocks)] for _ in range(3))
    cap = _capture_buffers(torch, pkg, info, nblocks, nch, dev)
    parts = 4 if schedule == "persistent_parts" else 0
    if persistent:
        pipe.plls_launch(nblocks, stream=s_pll)
    for b in range(nblocks):
        if b >= 2:
            s_fe.wait_event(post_done[b - 2])
        if parts and b == 0:
            pipe.frontend_pre_parts(iq[b], parts, stream=s_fe)    # the fill: the gated kernel variants
            pipe.fm_demod(cap["fm"][b], stream=s_fe)
            pipe.mono(cap["mono"][b], stream=s_fe)
        else:
            pipe.frontend(iq[b], stream=s_fe)
            pipe.fm_demod(cap["fm"][b], stream=s_fe)
            pipe.mono(cap["mono"][b], stream=s_fe)
            pipe.pre(stream=s_fe)
            if persistent:
                pipe.plls_signal(stream=s_fe)
        if persistent:
            pipe.plls_wait(stream=s_post)
        else:
            pre_done[b].record(s_fe)
            s_pll.wait_event(pre_done[b])
            pipe.plls(stream=s_pll)
            pll_done[b].record(s_pll)
            s_post.wait_event(pll_done[b])
        pipe.stereo_post(cap["lr"][b], stream=s_post)
        pipe.rds_post(cap["clean"][b], bits=True, stream=s_post)
        with torch.cuda.stream(s_post):
            for k in ("offset", "nsym", "symbols", "nbits", "bits"):
                cap[k][b].copy_(getattr(pipe, k))
        post_done[b].record(s_post)
    torch.cuda.synchronize(dev)
    if persistent:
        ms = pipe.plls_report(stream=s_pll)                # raises if a block's wait timed out
        assert len(ms) == nblocks
    host = {k: v.cpu().numpy() for k, v in cap.items()}
    pipe.close()
    bench.destroy_masked_streams(torch, pkg, dev, created)
    return host


def _kinds_a(synth):
    """Every kind of synth.KINDS at least twice among the 67 channels, the rest normal; hostile
    channels on both sides of 63 / 64 and in the partly filled last wave."""
    kinds = ["normal"] * NCH_A
    hostile = [k for k in synth.KINDS if k != "normal"]
    slots = [2 + 3 * i for i in range(len(hostile))] + [38 + 3 * i for i in range(len(hostile) - 1)] + [66]
    for i, s in enumerate(slots):
        kinds[s] = hostile[i % len(hostile)]
    assert all(kinds.count(k) >= 2 for k in synth.KINDS)
    return kinds


def _fit_cus(pipe):
    """The widest of the bench's PLL CU ranges that keeps the launch's workgroups resident."""
    for n in (64, 32, 16):
        try:
            if pipe.plls_fits(n)["fits"]:
                return n
        except Exception:
            continue
    pytest.fail("the persistent PLL launch fits none of CUs [0, 64), [0, 32), [0, 16)")


@pytest.fixture(scope="module", params=MODES)
def mode_mismatches(request, gpu, pkg, synth, tmp_path_factory):
    """All three schedules of one mode on the same 67 x 9 input; one oracle pass checks them."""
    torch, bench, dev = gpu
    mode = request.param
    probe = pkg.Pipeline(NCH_A, mode=mode, rds_on=True, device=0)
    info = probe.info
    n_cu = _fit_cus(probe)
    probe.close()
    # one wave per workgroup (6 waves on n_cu CUs), the register-prefetch lane-pair loop; the table
    # only where block_if doubles fit 64 KiB
    plan = {"wg_waves": 1, "staged": False, "tab_ok": TAB_OK[mode], "lds": 8 * info.block_if if TAB_OK[mode] else 0}
    kinds = _kinds_a(synth)
    iq = _make_input(torch, synth, info, NCH_A, NB_A, dev, kinds, seed=11 + mode)
    tmp = str(tmp_path_factory.mktemp(f"mode{mode}"))
    np.save(os.path.join(tmp, "iq.npy"), iq.cpu().numpy())
    ran = []
    for sch in SCHEDULES:
        host = _run_schedule(gpu, pkg, iq, mode, sch, n_cu, plan)
        if host is None:
            continue
        ran.append(sch)
        for k, v in host.items():
            np.save(os.path.join(tmp, f"{sch}_{k}.npy"), np.ascontiguousarray(v))
    del iq
    workers = max(1, min(16, os.cpu_count() or 1))
    step = (NCH_A + workers - 1) // workers
    jobs = [(tmp, lo, min(NCH_A, lo + step), mode, NB_A) for lo in range(0, NCH_A, step)]
    bad = {sch: [] for sch in ran}
    with cf.ProcessPoolExecutor(workers, mp_context=mp.get_context("spawn")) as ex:
        for r in ex.map(_check, jobs):
            for sch, v in r.items():
                bad[sch].extend(v)
    return mode, bad


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_mode_schedules_bit_exact(mode_mismatches, schedule):
    mode, bad = mode_mismatches
    if schedule not in bad:
        pytest.skip("no CU-masked streams: the bench does not run the persistent PLL without them")
    assert not bad[schedule], f"mode {mode} {schedule}: {len(bad[schedule])} mismatches, first: {bad[schedule][:10]}"


# b: packed groups. 512 channels = 32 waves on an 8-CU PLL stream, in groups of four waves: block 0
# through frontend_pre_parts (pll_run_split<true, TAB, true>), blocks 1-3 the staged loop
NCH_B, NB_B, CUS_B = 512, 4, 8
ORACLE_B = (0, 31, 32, 255, 256, 511)


def _kinds_b(synth):
    """Wave 1 (channels 32-63) holds every hostile kind; a second set straddles waves 7 and 8 (255 /
    256) and a third sits in the last wave. Returns (kinds, one channel of each hostile kind)."""
    kinds = ["normal"] * NCH_B
    hostile = [k for k in synth.KINDS if k != "normal"]
    second = list(range(250, 255)) + list(range(257, 262))
    for i, k in enumerate(hostile):
        kinds[33 + i] = k
        kinds[second[i]] = k
        kinds[490 + 2 * i] = k
    assert all(kinds[c] == "normal" for c in ORACLE_B)
    return kinds, [33 + i for i in range(len(hostile))]


@pytest.mark.parametrize("mode", MODES)
def test_packed_groups_staged_loop(gpu, pkg, synth, oracle, mode):
    """The four-wave groups of the 2048- and 4096-channel capacity lines in modes 1-3: every channel
    equals the one-stream pipeline on the same bytes, and channels 0, 31, 32, 255, 256, 511 and one
    channel of each hostile kind equal the oracle. Modes 1 and 3: no table; mode 2: the 64 000-byte
    table beside the staged loop's ring in one CU's LDS."""
    torch, bench, dev = gpu
    kinds, hostile_ch = _kinds_b(synth)
    och = sorted(set(ORACLE_B) | set(hostile_ch))
    pipe = pkg.Pipeline(NCH_B, mode=mode, rds_on=True, device=0)
    info = pipe.info
    fits = pipe.plls_fits(CUS_B)
    plan = pipe.plls_plan(CUS_B)
    assert plan == {"wg_waves": 4, "staged": True, "tab_ok": TAB_OK[mode],
                    "lds": 64000 if mode == 2 else 0}, f"mode {mode}: {plan} {fits}"
    assert fits["waves"] == 32 and fits["groups"] == 8 and fits["fits"], fits
    iq = _make_input(torch, synth, info, NCH_B, NB_B, dev, kinds, seed=23 + mode, first_channel=700)
    one = pkg.Pipeline(NCH_B, mode=mode, rds_on=True, device=0)       # the one-stream pipeline on the same bytes
    seq = {k: [] for k in KEYS}
    for b in range(NB_B):
        one.frontend(iq[b])
        seq["fm"].append(one.fm_demod()[och].cpu().numpy())
        seq["mono"].append(one.mono()[och].cpu().numpy())
        seq["lr"].append(one.stereo().cpu().numpy())
        seq["clean"].append(one.rds().cpu().numpy())
        for k in ("offset", "nsym", "symbols", "nbits", "bits"):
            seq[k].append(getattr(one, k).cpu().numpy().copy())
    one.close()
    created: list[int] = []
    try:
        s_fe, s_pll, s_post, _ = bench.cu_masked_streams(torch, pkg, dev, str(CUS_B), created, all_cus=False)
    except (RuntimeError, AttributeError):
        pipe.close()
        pytest.skip("no CU-masked streams: the bench does not run the persistent PLL without them")
    och_t = torch.tensor(och, dtype=torch.int64, device=dev)
    fm_all = torch.empty(NCH_B, info.block_if, dtype=torch.float32, device=dev)
    mono_all = torch.empty(NCH_B, info.n_audio, dtype=torch.int16, device=dev)
    cap = _capture_buffers(torch, pkg, info, NB_B, NCH_B, dev)
    del cap["fm"], cap["mono"]
    fm_keep, mono_keep = [], []
    post = [torch.cuda.Event() for _ in range(NB_B)]
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(torch.cuda.Stream(dev)):    # nothing on the null stream while the launch waits
        pipe.plls_launch(NB_B, stream=s_pll)
        for b in range(NB_B):
            if b >= 2:
                s_fe.wait_event(post[b - 2])
            if b == 0:
                pipe.frontend_pre_parts(iq[b], 4, stream=s_fe)
            else:
                pipe.frontend(iq[b], stream=s_fe)
            pipe.fm_demod(fm_all, stream=s_fe)
            pipe.mono(mono_all, stream=s_fe)
            with torch.cuda.stream(s_fe):
                fm_keep.append(fm_all[och_t])
                mono_keep.append(mono_all[och_t])
            if b > 0:
                pipe.pre(stream=s_fe)
                pipe.plls_signal(stream=s_fe)
            pipe.plls_wait(stream=s_post)
            pipe.stereo_post(cap["lr"][b], stream=s_post)
            pipe.rds_post(cap["clean"][b], bits=True, stream=s_post)
            with torch.cuda.stream(s_post):
                for k in ("offset", "nsym", "symbols", "nbits", "bits"):
                    cap[k][b].copy_(getattr(pipe, k))
            post[b].record(s_post)
        s_post.synchronize()
        ms = pipe.plls_report(stream=s_pll)            # raises if a block's wait timed out
    torch.cuda.synchronize(dev)
    assert len(ms) == NB_B
    got = {k: v.cpu().numpy() for k, v in cap.items()}
    got_fm = np.stack([t.cpu().numpy() for t in fm_keep])
    got_mono = np.stack([t.cpu().numpy() for t in mono_keep])
    iq_host = iq[:, och_t].cpu().numpy()
    pipe.close()
    bench.destroy_masked_streams(torch, pkg, dev, created)
    bad = []
    for b in range(NB_B):
        for k in ("lr", "clean", "offset", "nsym", "symbols", "nbits", "bits"):
            a, r = got[k][b], seq[k][b]
            if k == "clean":
                a, r = a.view(np.uint32), r.view(np.uint32)
            rows = np.nonzero((a != r).reshape(NCH_B, -1).any(axis=1))[0]
            if rows.size:
                bad.append(f"{k} b{b} vs one-stream: channels {rows[:8].tolist()} ({rows.size})")
    sub = {"fm": got_fm, "mono": got_mono, **{k: got[k][:, och] for k in KEYS if k not in ("fm", "mono")}}
    for j, c in enumerate(och):
        ref = oracle.run_channel(np.ascontiguousarray(iq_host[:, j]), mode, True)
        for b in range(NB_B):
            _compare(sub, b, c, ref, f"ch{c} ({kinds[c]}) b{b} vs oracle", bad, j=j)
    assert not bad, f"mode {mode}: {len(bad)} mismatches, first: {bad[:10]}"


# c: the engine. sdr_multi from a file runs each consumer's PLL as its own persistent launch
# (sdr_plls_launch_sel) on half of --cus
KINDS_C = ("normal", "silence", "noise", "pilot_offset", "weak")
CUS_C = 16


def _rds_text(tmp_path, ref) -> str:
    """The reference's frame layer (rds.cpp:181-189: start_frame_sync every 15 decoding blocks; host
    C++ rds_frame.cpp, pinned to the reference's text by tests/test_dropin_host.py) on the oracle's bits."""
    exe = tmp_path / "rds_text"
    if not exe.exists():
        gxx = shutil.which("g++")
        assert gxx is not None, "g++ (the host libraries are built with it)"
        subprocess.run([gxx, "-O1", "-std=c++17", "-I", str(ROOT / "include" / "dropin"),
                        str(ROOT / "tests" / "cpp" / "rds_text_driver.cpp"),
                        str(ROOT / "real-time-sdr_amd" / "host" / "rds_frame.cpp"), "-o", str(exe)], check=True)
    feed = "\n".join("-" if b is None else "".join(str(int(v)) for v in b) for b in ref["bits"]) + "\n"
    return subprocess.run([str(exe)], input=feed, capture_output=True, text=True, check=True, timeout=60).stderr


NB_C = 9


@pytest.mark.parametrize("mode", [1, 3])
def test_sdr_multi_modes_file_to_pcm_and_rds(gpu, pkg, synth, oracle, tmp_path, mode):
    """sdr_multi 5 --mode M from a file of right-rate bytes, 9 blocks: PREFIX.pcm of every channel and
    block bit-exact against the oracle (the stereo PLL's launch), PREFIX.rds equal to the reference's
    frame layer on the oracle's bits. That layer runs every 15 decoding blocks and 9 blocks hold three,
    so both texts are empty here: the RDS PLL's launch is only shown to end without a timeout."""
    nblocks = NB_C
    torch, bench, dev = gpu
    exe = ROOT / "real-time-sdr_amd" / "bin" / "sdr_multi"
    assert exe.exists(), "build with make"
    nch = len(KINDS_C)
    probe = pkg.Pipeline(nch, mode=mode, rds_on=True, device=0)
    info = probe.info
    half = CUS_C // 2
    for which, first in ((1, 0), (2, half)):            # the engine's two launches (sdr_multi_engine.cpp)
        assert probe.plls_plan(half, first_cu=first, which=which) == \
            {"wg_waves": 1, "staged": False, "tab_ok": 0, "lds": 0}
    iq = _make_input(torch, synth, info, nch, nblocks, dev, list(KINDS_C), seed=31 + mode).cpu().numpy()
    probe.close()
    np.ascontiguousarray(iq).tofile(tmp_path / "in.u8")
    r = subprocess.run([str(exe), str(nch), "--mode", str(mode), "--cus", str(CUS_C), "--out", str(tmp_path / "rx"),
                        "--in", str(tmp_path / "in.u8")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert f"{nch} channels x {nblocks} blocks" in r.stderr, r.stderr
    assert "PLLs persistent" in r.stderr, r.stderr
    pcm = np.fromfile(tmp_path / "rx.pcm", np.int16).reshape(nblocks, nch, 2 * info.n_audio)
    text = {}
    for line in (tmp_path / "rx.rds").read_text().splitlines():
        ch, _, rest = line.partition(": ")
        text.setdefault(int(ch.split()[1]), []).append(rest)
    for c in range(nch):
        ref = oracle.run_channel(np.ascontiguousarray(iq[:, c]), mode, True)
        for b in range(nblocks):
            assert np.array_equal(pcm[b, c], ref["stereo"][b]), f"stereo ch{c} ({KINDS_C[c]}) block {b}"
        want = _rds_text(tmp_path, ref)
        assert "".join(ln + "\n" for ln in text.get(c, [])) == want, f"RDS text ch{c} ({KINDS_C[c]})"
