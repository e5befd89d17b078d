#!/usr/bin/env python3
"""Throughput benchmark of the MI355X FM/RDS hot path (BASELINE.json metric).

One step = one block (73 500 I/Q pairs = 30.6 ms of signal) of every channel through the full
reference pipeline of `project 0 r` plus the mono stage: RF front end (u8 I/Q -> FIR /10 ->
discriminator), mono audio, stereo audio (pilot PLL, mixer, resamplers), RDS DSP (BPF, squaring,
PLL, mixer, 247/640 resampler, RRC) and RDS bit recovery (cdr, slicer, Manchester, differential).
Channels are independent and sharded across GPUs (weak scaling: 1024 channels per GPU, one process
per GPU); inputs are synthetic FM multiplex I/Q, 1024 distinct channels per GPU generated on the
device (synth.TorchMultiplexBatch) and resident in HBM before the timed region.

Three HIP streams per GPU mirror the reference's three threads (project.cpp:134-136): the front end
produces block b+1 while the stereo and RDS chains consume block b, ordered by events exactly like
the ThreadSafeQueue protocol (include/threadsafequeue.h:24-74). With N > 1 each block-step's stereo
audio and RDS bits are gathered to rank 0 over RCCL (xGMI) on a fourth, non-blocking stream.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--channels C] [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times the K steps and prints the result line (value, ms_per_step, and
the roofline / pll figures read from the timed steps' own stamps). --dump-outputs DIR also writes the
outputs of the last timed step (mono, stereo, rds_clean, rds_bits, rds_nbits; one row per channel,
float32) as DIR/<name>.npy; the input is seeded, so two builds can be compared array for array.
The set-up generates min(W + K, INPUT_RING = 160) input blocks; a longer run reads them round (block b
is block b % 160), so its set-up time and memory do not grow with K.
--full adds, after the timed steps: the bit-for-bit check of 8 channels against the oracle (`verified`),
the CPU baselines, the isolated front-end and HBM copy timings and the queue-plumbed receiver
(--no-cpu-baseline / --no-isolated leave parts of those out).
With --gpus N > 1 and no WORLD_SIZE in the environment, bench.py starts N ranks itself
(torch.distributed.run, 127.0.0.1) and exits with their status; the driver may also launch it
under torch.distributed.run directly.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import json
import multiprocessing as mp
import os
import pathlib
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent
HBM_PEAK_GBS = 8000.0           # MI355X HBM3E spec (MI355X_MICROARCH.md, chip-level parameters)
FP32_VECTOR_PEAK_TF = 157.3     # MI355X FP32 vector (packed) peak, TFLOP/s
METRIC = "IQ MSamples/s/node (mono+stereo+RDS), 1/2/4/8 GPU; HBM GB/s %peak"
VERIFY_CHANNELS = 8             # channels of rank 0 whose outputs are checked after the timed run
DUMP_MAX_BYTES = 60 << 20       # --dump-outputs: all arrays together (float32) stay below 64 MB
# Distinct input blocks resident in HBM. A run of more blocks (warm-up + steps) reads them round, block b
# being block b % INPUT_RING, so that its set-up time (~17 ms to generate a block of 1024 channels) and
# its memory (150 MB per block) do not grow with --steps. The default run (140 blocks) does not wrap.
INPUT_RING = 160


def _load_pkg():
    import importlib.util
    d = ROOT / "real-time-sdr_amd"
    if "real_time_sdr_amd" in sys.modules:
        return sys.modules["real_time_sdr_amd"]
    spec = importlib.util.spec_from_file_location("real_time_sdr_amd", d / "__init__.py",
                                                  submodule_search_locations=[str(d)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["real_time_sdr_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------ rank launcher
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(args, argv: list[str]) -> int:
    """bench.py --gpus N (N > 1) without WORLD_SIZE: start N ranks with torch.distributed.run as a
    CHILD process (never exec: nothing here has touched the GPU, and the ranks must start clean),
    one per GPU, and return their exit status. Fails if fewer than N GPUs are visible."""
    if args.backend == "nccl":
        import torch
        visible = torch.cuda.device_count()      # does not initialise the GPU on this image
        if visible < args.gpus:
            print(f"bench: --gpus {args.gpus} but only {visible} GPU(s) visible", file=sys.stderr)
            return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", str(pathlib.Path(__file__).resolve()),
           *argv]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


# ------------------------------------------------------------------------------ GPU stepper
def pll_cus(nch: int, fits, ncu: int = 256) -> int:
    """CUs for the PLL stream: 1, 2 or 4 PLL waves per CU, whichever bounds the block period least
    by a two-term model fitted to round 5's lines (profiles/r05/coal/, capacity/): the PLL's step at
    k waves per CU (209, 233, 263 shader cycles; 7350 steps at ~2.3 GHz) against the side chain's
    ~0.106 ms x channels / (CUs left); at equal periods fewer waves per CU, then fewer CUs. 1024
    channels -> 64 CUs (one wave per CU, the headline), 2048 -> 32 and 4096 -> 64 (four: the packed
    groups' LDS-staged loop). Only CU counts the library says a persistent launch can hold are
    candidates: fits(n) asks sdr_plls_fits whether every workgroup is resident on CUs [0, n) at once
    (a 48-CU mask falls unevenly on the shader engines and once left a 1536-channel launch waiting
    until its bounded waits expired, profiles/r05/coal/forced/)."""
    waves = 2 * ((2 * nch + 63) // 64)
    best = None
    for cus in range(8, 129, 8):
        k = (waves + cus - 1) // cus
        if k > 4 or not fits(cus):
            continue
        cyc = 209.0 if k <= 1 else 233.0 if k <= 2 else 263.0
        period = max(7350 * cyc / 2.3e6, 0.106 * nch / (ncu - cus))
        key = (round(period, 9), k, cus)
        if best is None or key < best[0]:
            best = (key, cus)
    return best[1] if best else 64


def cu_masked_streams(torch, pkg, dev, spec: str, created: list, all_cus: bool = True):
    """(fe, pll, post, all) streams through the C ABI (sdr_stream_create_cu_range): the PLL stream
    on CUs [0, n), front end and post on the rest, and one stream over every CU for the pipeline's
    fill and drain (the first block's pre-PLL work and the last block's post-PLL work, when the PLL
    CUs have nothing else to do). Every masked stream gets its own hardware queue. The runtime
    creates these streams blocking (hipExtStreamCreateWithCUMask has no flags), so nothing in the
    timed loop may run on the legacy null stream: the RCCL gather gets its own non-blocking torch
    stream."""
    import ctypes as C
    n = int(spec)
    L = pkg.lib()
    L.sdr_stream_create_cu_range.restype = C.c_int
    L.sdr_stream_create_cu_range.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    out = []
    ranges = ((0, n, 1), (0, n, 0), (0, n, 1)) + (((0, ncu, 0),) if all_cus else ())
    for lo, hi, exclude in ranges:
        h = C.c_void_p()
        rc = L.sdr_stream_create_cu_range(C.byref(h), dev.index, lo, hi, exclude)
        if rc != 0:
            raise RuntimeError(f"sdr_stream_create_cu_range: {rc} {L.sdr_last_error()}")
        created.append(h.value)
        out.append(torch.cuda.ExternalStream(h.value, device=dev))
    if not all_cus:
        out.append(None)
    return tuple(out)


def destroy_masked_streams(torch, pkg, dev, created: list) -> None:
    """sdr_stream_destroy the streams cu_masked_streams made (torch does not own them)."""
    import ctypes as C
    if not created:
        return
    torch.cuda.synchronize(dev)
    L = pkg.lib()
    L.sdr_stream_destroy.restype = C.c_int
    L.sdr_stream_destroy.argtypes = [C.c_void_p]
    while created:
        L.sdr_stream_destroy(C.c_void_p(created.pop()))


def _synth_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sdr_synth", ROOT / "real-time-sdr_amd" / "synth.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_input(torch, nch: int, nblocks: int, first_channel: int, device, kinds=None, seed: int = 0):
    """[nblocks][nch][2*73500] u8 on the device, nch distinct channels generated there
    (synth.TorchMultiplexBatch). Rows are padded to a multiple of 16 bytes (147008 for 147000): the
    front end then stages whole 16-byte I/Q groups."""
    synth = _synth_module()
    row = 2 * synth.BLOCK_IQ
    d = torch.empty((nblocks, nch, (row + 15) // 16 * 16), dtype=torch.uint8, device=device)[:, :, :row]
    gen = synth.TorchMultiplexBatch(torch, nch, first_channel, device, kinds=kinds, seed=seed)
    for b in range(nblocks):
        gen.next_block(out=d[b])
    torch.cuda.synchronize(device)
    return d


class GpuStepper:
    """The 1-GPU schedule of one rank: libsdr_amd.so's stage API on three HIP streams."""

    def __init__(self, args, nch: int, first: int, local: int, nblocks: int):
        import torch
        self.torch = torch
        self.pkg = pkg = _load_pkg()
        self.args, self.nch, self.nblocks, self.first = args, nch, nblocks, first
        self.dev = dev = torch.device("cuda", local)
        torch.cuda.set_device(dev)
        # the input is generated at the end of the set-up, right before the warm-up, so the GPU goes
        # from that load into the warm-up without the set-up's idle gap (shader clock 2306-2320 ->
        # 2312-2325 MHz, 0.7057-0.7076 -> 0.7032-0.7063 ms per step over 3 interleaved pairs at the
        # driver's 20/5, profiles/r06/input_last_ab.txt); SDR_BENCH_INPUT_LAST=0: first, as before
        self.input_last = os.environ.get("SDR_BENCH_INPUT_LAST", "1") == "1"
        self.ring = min(nblocks, INPUT_RING)      # input blocks generated; block b reads b % ring
        if not self.input_last:
            self.iq = make_input(torch, nch, self.ring, first_channel=first, device=dev)
        fast = args.numerics == "fast"
        self.fast = fast
        self.pipe = pkg.Pipeline(nch, mode=0, rds_on=True, device=local,
                                 flags=pkg.FLAG_FAST_FRONTEND if fast else 0)
        self.info = info = self.pipe.info
        # Three streams, one HIP hardware queue each (GPU_MAX_HW_QUEUES is 4): front end + mono +
        # the FIRs feeding both PLLs; both PLLs in one dispatch; everything after the PLLs. The
        # serial PLLs bound the step, so they run back to back across blocks while the other
        # streams fill the chip. SDR_BENCH_PRIO (A/B): streams (fe, pll, post) at high priority.
        prio = set(filter(None, os.environ.get("SDR_BENCH_PRIO", "").split(",")))
        s_fe, s_pll, s_post = (torch.cuda.Stream(dev, priority=-1 if n in prio else 0)
                               for n in ("fe", "pll", "post"))
        s_all = None
        # SDR_BENCH_CUMASK=<n> (0 = no masks): the PLL stream gets CUs [0, n), the front-end and
        # post streams the complement, so that no other kernel shares a CU's issue slots with the
        # PLL's waves (profiles/r01/ab_cumask.txt). Default: pll_cus(nch).
        self.created: list[int] = []
        ncu = torch.cuda.get_device_properties(dev).multi_processor_count
        cu_spec = os.environ.get("SDR_BENCH_CUMASK") or str(
            pll_cus(nch, lambda n: self.pipe.plls_fits(n)["fits"], ncu))
        if cu_spec not in ("", "0"):
            try:
                # the all-CU fill/drain stream is a fourth dedicated hardware queue: at N > 1 RCCL's
                # streams join the pool queues, so ranks keep three masked streams (a fifth queue
                # starved the front end at N = 1)
                world = int(os.environ.get("WORLD_SIZE", "1"))
                s_fe, s_pll, s_post, s_all = cu_masked_streams(torch, pkg, dev, cu_spec, self.created,
                                                               all_cus=world == 1)
            except (RuntimeError, ValueError, AttributeError) as exc:   # plain streams, reported
                print(f"bench: CU-masked streams unavailable ({exc}); unmasked streams", file=sys.stderr)
                destroy_masked_streams(torch, pkg, dev, self.created)
                cu_spec = ""
        self.cu_spec = cu_spec
        self.s_fe, self.s_pll, self.s_post = s_fe, s_pll, s_post
        # SDR_BENCH_EDGES=0: the first and last block of a phase stay on their masked streams
        self.s_all = s_all if os.environ.get("SDR_BENCH_EDGES", "1") != "0" else None
        # (not done: running the last block's stereo and RDS post stages side by side on a fifth
        # CU-masked stream. A fifth dedicated hardware queue starves the front-end stream: the PLL then
        # idles ~1 ms per 20 blocks waiting for input, 0.714 -> 0.78 ms/step, profiles/r03/drain2_ab.txt)
        self.phase = (0, -1)        # first and last block index of the current phase
        # SDR_BENCH_FILL_PARTS (default 4, 1 = off): the first block of a persistent phase in that
        # many sample ranges (sdr_frontend_pre_parts), so the PLL starts on its first range
        self.fill_parts = int(os.environ.get("SDR_BENCH_FILL_PARTS", "4"))
        self.parts_block = -1
        # SDR_BENCH_FILL_NEXT (A/B): what the second block's front end waits for. "parts" (default,
        # round 6): the first block's parts only (that block's mono stage runs on the all-CU stream
        # after them); "mono" (round 5): the parts and then the mono stage on the front-end stream,
        # ~70 us later. The PLL waited for the second block's input 0.17 ms per phase with "mono",
        # 0.09 with "parts" (−0.4 % per step at equal shader clock, 3 interleaved triples,
        # profiles/r06/fill_next/ab.txt). It cannot start before
        # the parts: it continues their tails (the front end's I/Q tail and discriminator state, the
        # FIRs' histories); "all": "parts", and the second block's front end and pre-PLL FIRs on the
        # all-CU stream too
        self.fill_next = os.environ.get("SDR_BENCH_FILL_NEXT", "parts")
        self.ev_fork, self.ev_join = torch.cuda.Event(), torch.cuda.Event()
        # SDR_BENCH_PLL=persistent (default): one PLL dispatch per phase (warm-up, timed) that waits
        # for each block's device flag (sdr_plls_launch/_signal/_wait); "dispatch": one sdr_plls
        # dispatch per block, ordered by events. The persistent kernel's waves spin until a later
        # dispatch on the front-end stream publishes the block, so it may only run where that
        # dispatch cannot queue behind it: the PLL stream must own its hardware queue. A CU-masked
        # stream does (the runtime gives every stream with a CU mask a dedicated HSA queue instead
        # of sharing one from the pool), plain streams do not (GPU_MAX_HW_QUEUES = 4 pool queues are
        # shared by the torch streams, the gather stream and RCCL's): without masks -> dispatch.
        # All of a persistent launch's waves must be resident on the PLL stream's CUs at once: the
        # library checks that (and the stream's own hardware queue) and refuses the launch before any
        # dispatch otherwise (4096 channels on 64 CUs); the blocks then run as per-block dispatches.
        want = os.environ.get("SDR_BENCH_PLL", "persistent")
        self.persist = want == "persistent" and bool(self.created)
        why = ("" if want != "persistent" or self.persist else " (no CU-masked streams: persistent PLL not safe)")
        self.pll_mode = ("persistent" if self.persist else "dispatch") + why
        self.s_gather = torch.cuda.Stream(dev)       # torch pool streams are non-blocking
        self.mono = torch.empty(nch, info.n_audio, dtype=torch.int16, device=dev)
        self.lr = [torch.empty(nch, 2 * info.n_audio, dtype=torch.int16, device=dev) for _ in range(2)]
        self.bits = [torch.empty(nch, pkg.SDR_MAX_BITS, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.clean = torch.empty(nch, info.n_rds, dtype=torch.float32, device=dev)
        ev = lambda: torch.cuda.Event(enable_timing=False)  # noqa: E731
        tev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
        self.fe_start, self.fe_end = [tev() for _ in range(nblocks)], [tev() for _ in range(nblocks)]
        self.pll_start, self.pll_done = [tev() for _ in range(nblocks)], [tev() for _ in range(nblocks)]
        self.gather_done = [ev() for _ in range(nblocks)]
        self.pre_done, self.post_done = [tev() for _ in range(nblocks)], [tev() for _ in range(nblocks)]
        self.post_dsp_done = [ev() for _ in range(nblocks)]   # block b's post DSP (before its captures)
        if self.input_last:
            self.iq = make_input(torch, nch, self.ring, first_channel=first, device=dev)
        # the front end of block b also waits for block b-2's whole post stream work (the RDS chain
        # after its mixer, the output copies and captures included), not only for the library's own
        # parity release (its readers' first kernels): the front end then runs beside the PLL alone
        # instead of beside block b-2's RDS chain -- 0.111 against 0.140 ms per front end and 0.6954-
        # 0.7088 against 0.7115-0.7189 ms per step, 3 interleaved pairs (profiles/r05/fe_wait_ab.txt).
        # SDR_BENCH_FE_WAIT=library (A/B): the parity release alone.
        # Past 1024 channels per GPU the side chain, not the PLL, sets the period, and that wait
        # lengthens its critical path (2048 channels: 143.0 against 148.7 GS/s), so there the
        # release alone orders the front end.
        self.fe_waits_post = os.environ.get("SDR_BENCH_FE_WAIT", "post" if nch <= 1024 else "library") == "post"
        # that wait covers block b-2's post DSP only, not its output captures (SDR_BENCH_FE_GATE=all: those too)
        self.fe_gate_all = os.environ.get("SDR_BENCH_FE_GATE", "dsp") == "all"
        # outputs of a few channels, captured on the producing streams for the check after timing
        nv = min(VERIFY_CHANNELS, nch)
        self.vsel = torch.tensor(sorted({int(round(i * (nch - 1) / max(1, nv - 1))) for i in range(nv)}),
                                 dtype=torch.int64, device=dev)
        nv = self.vsel.numel()
        self.cap_mono = torch.empty(nblocks, nv, info.n_audio, dtype=torch.int16, device=dev)
        self.cap_lr = torch.empty(nblocks, nv, 2 * info.n_audio, dtype=torch.int16, device=dev)
        self.cap_bits = torch.empty(nblocks, nv, pkg.SDR_MAX_BITS, dtype=torch.uint8, device=dev)
        self.cap_nbits = torch.empty(nblocks, nv, dtype=torch.int32, device=dev)
        self.cap_g = None           # receiving rank: the same rows of every rank's gathered block

    def outputs_spec(self):
        return {"lr": ((self.nch, 2 * self.info.n_audio), self.torch.int16),
                "bits": ((self.nch, self.pkg.SDR_MAX_BITS), self.torch.uint8)}

    def prepare_phase(self, nblocks: int) -> None:
        """Before the timer: the persistent launch's bookkeeping (stamp arrays reset), so the timed
        region starts with the launch and the first front end instead of four memsets."""
        # the front-end kernels of the timed blocks record their own dispatch stamps (the roofline's
        # average launch time: the kernel alone, as a rocprofv3 kernel trace times it)
        self.pipe.frontend_timing(nblocks)
        if self.persist:
            self.pipe.plls_prepare(nblocks, stream=self.s_pll)
            self.torch.cuda.synchronize(self.dev)

    def begin_phase(self, nblocks: int) -> None:
        """Before the warm-up and before the timed blocks: the persistent PLL dispatch of the phase.
        A launch the library refuses (before any dispatch: its waves would not all be resident on the
        PLL stream's CUs) turns the bench to per-block dispatches, named in `pll.mode`."""
        if self.persist:
            try:
                self.pipe.plls_launch(nblocks, stream=self.s_pll)
            except self.pkg.SdrError as exc:
                self.persist = False
                self.pll_mode = f"dispatch (persistent launch refused: {exc})"
        self.next_first = True
        self.phase_len = nblocks

    @property
    def launch_pending(self) -> bool:
        """A phase's persistent PLL launch may be waiting for blocks (until the phase's synchronize)."""
        return self.persist

    def prime_gather(self, gather) -> None:
        """N > 1, before the first phase: one untimed gather round (RCCL's lazy connection set-up runs
        here, not beside a pending persistent launch) and the receiving rank's capture buffers, so
        that inside a phase the per-step gather allocates nothing."""
        torch = self.torch
        with torch.cuda.stream(self.s_gather):
            got = gather(lr=self.lr[0], bits=self.bits[0])
            if got is not None:
                self._alloc_capture(got)
        torch.cuda.synchronize(self.dev)

    def step(self, b: int, gather=None) -> None:
        torch, pipe = self.torch, self.pipe
        s_fe, s_pll, s_post = self.s_fe, self.s_pll, self.s_post
        # pipeline fill and drain: nothing runs beside the first block's pre-PLL work or the last
        # block's post-PLL work, so those take every CU (the all-CU stream), ordered by events
        first = getattr(self, "next_first", False)
        self.next_first = False
        if first:
            self.phase = (b, b + getattr(self, "phase_len", 1) - 1)
        edge_fe = self.s_all is not None and (
            b == self.phase[0] or (self.fill_next == "all" and b == self.phase[0] + 1 == self.parts_block + 1))
        edge_post = self.s_all is not None and b == self.phase[1]
        if edge_fe:
            s_fe = self.s_all
        if edge_post:
            s_post = self.s_all
            s_post.wait_event(self.post_done[b - 1]) if b >= 1 else None
        # the front end of block b reuses block b-2's parity: both consumers must have released it
        # (threadsafequeue.h:29-31). The library orders that itself: sdr_frontend waits on its stream
        # for the release counts that block b-2's mono, stereo post and RDS mixer stored on theirs
        # (the RDS chain after its mixer and the output captures are not waited for)
        if b >= 2 and self.fe_waits_post:
            s_fe.wait_event((self.post_done if self.fe_gate_all else self.post_dsp_done)[b - 2])
        # that wait (a one-wave kernel) goes ahead of the timer, so fe_start..fe_end spans the
        # front-end kernel alone (the roofline's average launch time; frontend() then waits no more)
        pipe.release_wait(stream=s_fe)
        self.fe_start[b].record(s_fe)
        if first and self.persist and self.fill_parts > 1:
            # the pipeline fill: the phase's first block in sample ranges, each published to the
            # persistent PLL as soon as its front end and pre-PLL FIRs are done
            pipe.frontend_pre_parts(self.iq[b % self.ring], self.fill_parts, stream=s_fe)
            self.parts_block = b
        else:
            pipe.frontend(self.iq[b % self.ring], stream=s_fe)            # rffrontend.cpp:58-71
            self.fe_end[b].record(s_fe)
            pipe.pre(stream=s_fe)                             # stereo.cpp:74, :80 + rds.cpp:105-116
            if self.persist:                                  # stereo.cpp:77 + rds.cpp:119
                pipe.plls_signal(stream=s_fe)
        self.pre_done[b].record(s_fe)
        s_mono = s_fe
        if edge_fe:                                           # the rest of the phase's front ends follow it
            s_fe = self.s_fe
            s_fe.wait_event(self.pre_done[b])
            if self.fill_next == "mono" or b != self.parts_block:
                s_mono = s_fe
        pipe.mono(self.mono, stream=s_mono)                   # mono.cpp:34-42 (off the PLLs' critical path)
        with torch.cuda.stream(s_mono):
            torch.index_select(self.mono, 0, self.vsel, out=self.cap_mono[b])
        if self.persist:
            pipe.plls_wait(stream=s_post)
            self.pll_done[b].record(s_post)                   # the PLL's block b released (drain timing)
        else:
            s_pll.wait_event(self.pre_done[b])
            self.pll_start[b].record(s_pll)
            pipe.plls(stream=s_pll)
            self.pll_done[b].record(s_pll)
            s_post.wait_event(self.pll_done[b])
        if gather is not None and b >= 2:
            s_post.wait_event(self.gather_done[b - 2])        # lr/bits slot of block b-2 gathered
        lr, bits = self.lr[b % 2], self.bits[b % 2]
        # drain: the stereo post stage (its own buffers) beside the RDS one, on the post stream that
        # is idle by then (no fifth hardware queue: DESIGN.md 5)
        s_st = s_post
        if edge_post:
            s_st = self.s_post
            self.ev_fork.record(s_post)
            s_st.wait_event(self.ev_fork)
        pipe.stereo_post(lr, stream=s_st)                     # stereo.cpp:83-107
        pipe.rds_post(self.clean, bits=True, stream=s_post, bits_out=bits)   # rds.cpp:122-167
        if s_st is s_post:
            # the front end of block b + 2 waits for this, not for the output captures below
            self.post_dsp_done[b].record(s_post)
        with torch.cuda.stream(s_post):
            torch.index_select(bits, 0, self.vsel, out=self.cap_bits[b])
            torch.index_select(pipe.nbits, 0, self.vsel, out=self.cap_nbits[b])
        with torch.cuda.stream(s_st):
            torch.index_select(lr, 0, self.vsel, out=self.cap_lr[b])
        if s_st is not s_post:
            self.ev_join.record(s_st)
            s_post.wait_event(self.ev_join)
            self.post_dsp_done[b].record(s_post)
        self.post_done[b].record(s_post)
        if gather is not None:
            # final audio / bitstream gather to rank 0 over RCCL (xGMI), on its own non-blocking
            # stream so that the masked (blocking) streams never meet null-stream work
            with torch.cuda.stream(self.s_gather):
                self.s_gather.wait_event(self.post_done[b])
                got = gather(lr=lr, bits=bits)
                if got is not None:
                    self._capture_gathered(b, got)
                self.gather_done[b].record(self.s_gather)

    def _capture_gathered(self, b: int, got: dict) -> None:
        """Receiving rank: rows vsel of every rank's gathered lr / bits of block b, kept for the check
        after the timed region (the gather buffers are reused every block-step)."""
        torch = self.torch
        world = len(got["lr"])
        if self.cap_g is None:
            raise RuntimeError("gather capture buffers not allocated (prime_gather before the first phase)")
        for k in ("lr", "bits"):
            for r in range(world):
                torch.index_select(got[k][r], 0, self.vsel_g, out=self.cap_g[k][b, r])

    def _alloc_capture(self, got: dict) -> None:
        torch = self.torch
        world = len(got["lr"])
        d = got["lr"][0].device
        nv = self.vsel.numel()
        self.vsel_g = self.vsel.to(d)
        self.cap_g = {k: torch.empty((self.nblocks, world, nv) + tuple(got[k][0].shape[1:]), dtype=got[k][0].dtype,
                                     device=d) for k in ("lr", "bits")}

    def gathered_digests(self) -> list | None:
        """Receiving rank: per source rank, the digest of its gathered rows (compared with the digest
        the source rank computes over its own outputs, captured()['digest'])."""
        if self.cap_g is None:
            return None
        lr, bits = self.cap_g["lr"].cpu().numpy(), self.cap_g["bits"].cpu().numpy()
        return [_digest(lr[:, r], bits[:, r]) for r in range(lr.shape[1])]

    def synchronize(self) -> None:
        self.torch.cuda.synchronize(self.dev)

    def report(self, warmup: int, elapsed: float, steps: int) -> dict:
        """Kernel-level timings of the timed blocks (HIP events on the launching streams)."""
        info, nch = self.info, self.nch
        rng = range(warmup, self.nblocks)
        # the front-end kernel's own time per launch: earliest workgroup start to latest workgroup end
        # (sdr_frontend_timing, armed in prepare_phase); a block whose front end ran in parts (the
        # fill) has none. Without them, the HIP events around each launch on its stream.
        fe_ms = self.pipe.frontend_times()
        fe_src = "the kernel's own workgroup start/end stamps (sdr_frontend_timing)"
        if not fe_ms:
            fe_ms = [self.fe_start[b].elapsed_time(self.fe_end[b]) for b in rng if b != self.parts_block]
            fe_src = "HIP events around each launch"
        fe_avg_s = float(np.mean(fe_ms)) / 1e3
        fe_bytes = nch * (2 * info.block_iq + 4 * info.block_if)     # u8 I/Q in + f32 fm_demod out
        cyc = None
        timeline = None
        if self.persist:   # device-clock time of each block inside the timed phase's dispatch
            pll_ms = float(np.mean(self.pipe.plls_report(stream=self.s_pll)))
            cyc = self.pipe.plls_cycles(stream=self.s_pll)   # the waves' own shader-clock count
            ts, te = self.pipe.plls_timeline(stream=self.s_pll)
            if ts and te:
                # the timed phase on the device clock: the PLL span from block 0's signal to the last
                # block's end, the PLL's idle time between blocks (input not ready), and what the
                # host-timed phase spends outside the span (pipeline fill before block 0's PLL and
                # the last block's post stage after it)
                span = (te[-1] - ts[0]) * 1e-5
                gaps = [max(0, ts[j] - te[j - 1]) * 1e-2 for j in range(1, len(ts))]   # µs
                idle = sum(gaps) * 1e-3
                first, last = warmup, warmup + steps - 1
                phase = self.fe_start[first].elapsed_time(self.post_done[last])
                # drain: from the release of the PLL's last block (the post stream's wait) to the end
                # of its post stage; fill: the rest of the device phase before the PLL span (the
                # first block's front end and pre-PLL FIRs up to the PLL's first published range)
                drain = self.pll_done[last].elapsed_time(self.post_done[last])
                timeline = {"pll_span_ms": round(span, 4), "pll_idle_ms": round(idle, 4),
                            "pll_idle_us_by_block": [round(g, 1) for g in gaps],
                            "pll_block_us": [round((te[j] - ts[j]) * 1e-2, 1) for j in range(len(ts))],
                            "pll_period_us": [round((te[j] - te[j - 1]) * 1e-2, 1) for j in range(1, len(te))],
                            "pll_block_mhz": [round(m, 1) for m in self.pipe.plls_block_cycles(stream=self.s_pll)[1]],
                            "pll_block_cycles": [round(c, 1) for c in self.pipe.plls_block_cycles(stream=self.s_pll)[0]],
                            "outside_span_ms": round(elapsed * 1e3 - span, 4),
                            "device_phase_ms": round(phase, 4), "fill_ms": round(phase - span - drain, 4),
                            "fill_parts": self.fill_parts if self.parts_block == first else 1,
                            "fill_next": self.fill_next,
                            "drain_ms": round(drain, 4)}
                sides = self._fe_vs_pll(ts, te)
                if sides:
                    timeline["front_end_vs_pll_us"] = sides
        else:
            pll_ms = float(np.mean([self.pll_start[b].elapsed_time(self.pll_done[b]) for b in rng]))
        achieved = fe_bytes / fe_avg_s / 1e9
        redo = self._pll_redo()
        waves = self._pll_waves(info.block_if)
        kname = ("k_frontend_mfma" if self.fast else "k_frontend2") + " (u8 I/Q -> 101-tap FIR /10 on I,Q -> FM discriminator)"
        return {
            "roofline": {"kernel": kname, "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                         "traffic": _pmc_traffic(nch, self.args.numerics),
                         "algorithmic_bytes_per_launch": fe_bytes, "avg_launch_ms": round(fe_avg_s * 1e3, 4),
                         "launches_timed": len(fe_ms), "timed_by": fe_src},
            "pll": {"kernel": ("k_pll_multi: persistent, all blocks of the phase in one dispatch" if self.persist
                               else "k_pll: one dispatch per block") +
                              ", stereo 19 kHz + RDS 114 kHz PLLs (pll.cpp:4-61), 2 x channels serial chains",
                    "bound": "serial recurrence: block_if dependent steps per chain, " +
                             "a lane pair per chain (cos / sin lanes)" +
                             " (per-wave issue and dependent latency, DESIGN.md 4a)",
                    "mode": self.pll_mode,
                    "avg_launch_ms": round(pll_ms, 4), "ns_per_step": round(pll_ms * 1e6 / info.block_if, 2),
                    "share_of_step": round(pll_ms / (elapsed / steps * 1e3), 4),
                    **self._pll_issue(cyc),
                    **({"timeline": timeline} if timeline else {}),
                    **({"chunk_redo": redo} if redo else {}),
                    **({"waves": waves} if waves else {})},
        }

    def _fe_vs_pll(self, ts: list, te: list) -> dict | None:
        """Where each timed block's front end sat against the PLL (the same 100 MHz device clock:
        the front end's own workgroup stamps, the persistent launch's per-block stamps), medians over
        the phase's blocks j >= 2 (phase-relative; block 0 ran its front end in parts, untimed):
          release_to_fe: front-end start - PLL end of block j-2 (its parity's readers run after it),
          fe: the front end's span, fe_to_pll: PLL start of block j - front-end end (the pre-PLL FIRs
          and the signal; when the PLL waited for the block), pll_gap: PLL start of j - PLL end of j-1."""
        try:
            f0, f1 = self.pipe.frontend_stamps()
        except self.pkg.SdrError:
            return None
        off = 1 if self.parts_block == self.phase[0] else 0     # launch i = phase block i + off
        rows = {"release_to_fe": [], "fe": [], "fe_to_pll": [], "pll_gap": []}
        for i in range(len(f0)):
            j = i + off
            if j < 2 or j >= len(ts):
                continue
            rows["release_to_fe"].append((f0[i] - te[j - 2]) * 1e-2)
            rows["fe"].append((f1[i] - f0[i]) * 1e-2)
            rows["fe_to_pll"].append((ts[j] - f1[i]) * 1e-2)
            rows["pll_gap"].append((ts[j] - te[j - 1]) * 1e-2)
        if not rows["fe"]:
            return None
        out = {k: round(float(np.median(v)), 1) for k, v in rows.items()}
        out["max"] = {k: round(float(np.max(v)), 1) for k, v in rows.items()}
        return out

    @staticmethod
    def _pll_issue(cyc) -> dict:
        """The PLL's efficiency against its bound (one wave per SIMD issues one VALU per quad-cycle):
        VALU instructions per step from the committed counters, cycles per step measured live by the
        waves' own s_memtime, and issue_frac = 4 x VALU per step / cycles per step."""
        out = {}
        pc = _pll_counters()
        if cyc is not None and cyc[0] > 0:
            out["cycles_per_step"] = round(cyc[0], 1)
            out["shader_clock_mhz"] = round(cyc[1], 1)
        if pc:
            out["valu_per_step"] = pc.get("valu_per_step")
            out["counters"] = pc.get("source")
            if "cycles_per_step" in out and pc.get("valu_per_step"):
                out["issue_frac"] = round(4.0 * pc["valu_per_step"] / out["cycles_per_step"], 4)
        return out

    def _pll_waves(self, n: int) -> dict | None:
        """Diagnosis builds (-DSDR_PLL_WAVES=1) only: the persistent launch's waves (the timed phase)
        per job -- mean and slowest shader cycles per step inside their blocks, and the flag-poll
        time per block -- to tell a slow wave from the hand-off in the span's excess over the mean."""
        import ctypes as C
        f = getattr(self.pkg.lib(), "sdr_diag_pll_waves", None)
        if f is None or not self.persist:
            return None
        nmax, nf = 4096, 8
        c = (C.c_ulonglong * (nf * nmax))()
        nw = f(c, nmax)
        if nw <= 0:
            return None
        v = np.frombuffer(c, dtype=np.uint64).reshape(nmax, nf)[:nw].astype(np.float64)
        v = v[(v[:, 3] > 0) & (v[:, 2] > 0)]
        out = {}
        for job, name in ((1, "stereo_19k"), (2, "rds_114k")):
            w = v[v[:, 3] == job]
            if len(w) == 0:
                continue
            cyc = w[:, 0] / w[:, 2] / n
            poll_us = w[:, 1] / w[:, 2] * 1e-2
            out[name] = {"waves": int(len(w)), "cycles_per_step_mean": round(float(cyc.mean()), 2),
                         "cycles_per_step_max": round(float(cyc.max()), 2),
                         "cycles_per_step_min": round(float(cyc.min()), 2),
                         "poll_us_per_block_mean": round(float(poll_us.mean()), 2),
                         "poll_us_per_block_max": round(float(poll_us.max()), 2),
                         "spin_us_per_block_mean": round(float((w[:, 4] / w[:, 2] * 1e-2).mean()), 2),
                         "polls_unset_per_block": round(float((w[:, 5] / w[:, 2]).mean()), 2),
                         "blocks_flag_ready_frac": round(float((w[:, 6] / w[:, 2]).mean()), 3),
                         "flag_ahead_us_per_block": round(float((w[:, 7] / w[:, 2] * 1e-2).mean()), 2)}
        return out or None

    def _pll_redo(self) -> dict | None:
        """Diagnosis builds (-DSDR_PLL_COUNT=1) only: fraction of the PLL's 16-step chunks whose proof
        failed (per lane) and that a wave redid with the checked path, over warm-up and timed blocks."""
        import ctypes as C
        f = getattr(self.pkg.lib(), "sdr_diag_pll_counts", None)
        if f is None:
            return None
        c = (C.c_ulonglong * 10)()
        if f(c, 0) != 0 or c[0] == 0:
            return None
        return {"lane_chunks": c[0], "lane_fail_frac": c[1] / c[0], "wave_chunks": c[2],
                "wave_redo_frac": c[3] / max(c[2], 1),
                "lane_fail_by_reason": {"e_range": c[4], "e_bracket": c[5], "cos_sin_tie": c[6], "state": c[7]},
                "lane_fail_by_job": {"stereo_19k": c[8], "rds_114k": c[9]}}

    def isolated_frontend(self) -> dict:
        """Outside the timed region: the front-end kernel of both numerics modes alone on the GPU
        (one stream, the same resident inputs, 20 back-to-back launches), each as a roofline object
        whose launch time is the kernel's own (its workgroups' start / end stamps, sdr_frontend_times,
        as in the pipeline line); avg_call_ms_events: HIP events around the 20 calls, per call
        (kernel plus the gap between dependent dispatches)."""
        torch, pkg, nch, info = self.torch, self.pkg, self.nch, self.info
        fe_bytes = nch * (2 * info.block_iq + 4 * info.block_if)
        res = {}
        for name, flags in (("exact", 0), ("fast", pkg.FLAG_FAST_FRONTEND)):
            p2 = pkg.Pipeline(nch, mode=0, rds_on=True, device=self.dev.index, flags=flags)
            s2 = torch.cuda.Stream(self.dev)
            for b in range(min(self.nblocks, 3)):
                p2.frontend(self.iq[b], stream=s2)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 20
            p2.frontend_timing(reps)
            e0.record(s2)
            for b in range(reps):
                p2.frontend(self.iq[b % self.ring], stream=s2)
            e1.record(s2)
            torch.cuda.synchronize(self.dev)
            ms_calls = e0.elapsed_time(e1) / reps
            kern = p2.frontend_times(reps)
            ms = float(np.mean(kern)) if kern else ms_calls
            gbs = fe_bytes / (ms / 1e3) / 1e9
            res[name] = {"kernel": "k_frontend_mfma (int8 MFMA Toeplitz FIR)" if flags else "k_frontend2",
                         "bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(gbs / HBM_PEAK_GBS, 4), "traffic": _pmc_traffic(nch, name),
                         "avg_launch_ms": round(ms, 4), "launches_timed": len(kern),
                         "timed_by": "the kernel's own workgroup start/end stamps" if kern else "HIP events",
                         "avg_call_ms_events": round(ms_calls, 4)}
            if not flags:
                # exact mode is VALU-bound (f32 multiply and add per tap, no FMA): the same time
                # against the f32 vector peak (report the VALU fraction too)
                flops = nch * info.block_if * 2 * info.rf_taps * 2
                res[name]["valu"] = {"achieved_tflops": round(flops / (ms / 1e3) / 1e12, 2),
                                     "peak_tflops": FP32_VECTOR_PEAK_TF,
                                     "frac": round(flops / (ms / 1e3) / 1e12 / FP32_VECTOR_PEAK_TF, 4)}
            p2.close()
        res["hbm_copy"] = cp = self.copy_bandwidth()
        for name in ("exact", "fast"):   # against the rate a plain copy reaches on this box
            res[name]["frac_of_copy"] = round(res[name]["achieved"] / cp["achieved"], 4)
        return res

    def copy_bandwidth(self, nbytes: int = 1 << 31, reps: int = 10) -> dict:
        """Device-to-device copy of a 2 GiB buffer (read + write bytes / time) with the library's
        streaming copy kernel (sdr_hbm_copy): the HBM rate a plain stream reaches on this box, next
        to the nominal 8 TB/s peak."""
        torch, pkg = self.torch, self.pkg
        a = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        b = torch.empty_like(a)
        s2 = torch.cuda.Stream(self.dev)
        with torch.cuda.stream(s2):
            a.fill_(1)
            for _ in range(2):
                pkg.hbm_copy(b, a, stream=s2)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s2)
            for _ in range(reps):
                pkg.hbm_copy(b, a, stream=s2)
            e1.record(s2)
        torch.cuda.synchronize(self.dev)
        ms = e0.elapsed_time(e1) / reps
        del a, b
        return {"kernel": "k_hbm_copy (sdr_hbm_copy: one 16-byte element per lane, one workgroup per 4 KiB)",
                "bytes": 2 * nbytes,
                "achieved": round(2 * nbytes / (ms / 1e3) / 1e9, 1), "unit": "GB/s",
                "frac_of_peak": round(2 * nbytes / (ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4)}

    def captured(self) -> dict:
        """Host copies of the inputs and captured outputs of the checked channels."""
        sel = self.vsel.cpu().numpy()
        iq = self.iq[:, self.vsel].cpu().numpy()[np.arange(self.nblocks) % self.ring]   # [nblocks][nv][2*block_iq]
        lr, bits = self.cap_lr.cpu().numpy(), self.cap_bits.cpu().numpy()
        return {"channels": [int(c) for c in sel], "first_channel": self.first, "iq": iq,
                "mono": self.cap_mono.cpu().numpy(), "lr": lr, "bits": bits, "nbits": self.cap_nbits.cpu().numpy(),
                "digest": _digest(lr, bits)}

    def last_outputs(self, max_bytes: int = DUMP_MAX_BYTES) -> dict:
        """--dump-outputs: what the last timed step handed to a caller of the pipeline, as float32
        host arrays with one row per channel: mono and stereo PCM, rds_clean, the RDS bits (-1 past
        the nbits[channel] bits the row holds: the buffer is not written there) and nbits. Past
        max_bytes in all, the rows of a fixed, seeded choice of channels (`channels`)."""
        torch = self.torch
        b = self.nblocks - 1
        nbits = self.pipe.nbits
        col = torch.arange(self.pkg.SDR_MAX_BITS, device=self.dev)
        bits = torch.where(col[None, :] < nbits[:, None], self.bits[b % 2].to(torch.int32), -1)
        outs = {"mono": self.mono, "stereo": self.lr[b % 2], "rds_clean": self.clean, "rds_bits": bits,
                "rds_nbits": nbits}
        rows = max_bytes // (4 * sum(t[0].numel() for t in outs.values()))
        sel = None
        if rows < self.nch:
            sel = np.sort(np.random.Generator(np.random.PCG64(20240)).choice(self.nch, max(1, rows), replace=False))
            idx = torch.from_numpy(sel).to(self.dev)
            outs = {k: t.index_select(0, idx) for k, t in outs.items()}
        res = {k: t.cpu().numpy().astype(np.float32) for k, t in outs.items()}
        if sel is not None:
            res["channels"] = sel.astype(np.float64)
        return res

    def close(self) -> None:
        self.pipe.close()
        destroy_masked_streams(self.torch, self.pkg, self.dev, self.created)


def _digest(lr, bits) -> str:
    """SHA-256 over captured stereo audio and RDS bit rows ([blocks][channels][...])."""
    import hashlib
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(lr).tobytes())
    h.update(np.ascontiguousarray(bits).tobytes())
    return h.hexdigest()


def write_outputs(directory: str, outs: dict) -> None:
    """--dump-outputs DIR: one DIR/<name>.npy per output array of the last timed step."""
    d = pathlib.Path(directory)
    d.mkdir(parents=True, exist_ok=True)
    for name, a in outs.items():
        np.save(d / f"{name}.npy", np.ascontiguousarray(a))


def _pll_counters() -> dict | None:
    """Committed SQ counters of the PLL kernel (profiles/pll_counters.json, from a rocprofv3 --pmc
    pass with per-block PLL dispatch: PMC serialises dispatches, which the persistent launch cannot
    run under): VALU instructions and issue quad-cycles per PLL step."""
    try:
        return json.loads((ROOT / "profiles" / "pll_counters.json").read_text())
    except (OSError, ValueError):
        return None


def _pmc_traffic(nch: int, numerics: str):
    """HBM bytes per launch of the front end from rocprofv3 PMC passes (FETCH_SIZE x2 gfx950
    correction + WRITE_SIZE; tools/pmc_summary.py), committed under profiles/."""
    prof = ROOT / "profiles" / "pmc_frontend.json"
    try:
        pm = json.loads(prof.read_text())
        if pm.get("channels") == nch:
            return pm.get(numerics, {}).get("hbm_bytes_per_launch")
    except (OSError, ValueError):
        pass
    return None


# ------------------------------------------------------------------------------ rank path
_DIST_CALLS = ("barrier", "all_reduce", "reduce", "broadcast", "all_gather", "all_gather_into_tensor", "gather",
               "scatter", "reduce_scatter", "reduce_scatter_tensor", "all_to_all", "all_to_all_single", "send",
               "recv", "isend", "irecv", "gather_object", "all_gather_object", "broadcast_object_list",
               "batch_isend_irecv", "monitored_barrier")


class LaunchWindow:
    """The span of one phase from its persistent PLL launch to the phase's final synchronize. The
    PLL stream is CU-masked, hence blocking: anything that synchronises the device implicitly (a
    collective's set-up, a hipMalloc / hipFree of the caching allocator) would wait for the pending
    launch until its 5 s bound. Inside the window every torch.distributed call but the per-step
    gather (wrapped by gather()) raises; a device allocation or free made between arm() and check()
    (torch.cuda.memory_stats num_device_alloc / num_device_free, read outside the timed region:
    the call itself costs a fraction of a millisecond) fails the run."""

    def __init__(self, torch, dist, device, active: bool):
        self.torch, self.dist, self.active = torch, dist, active
        self.device = torch.device(device) if not isinstance(device, str) else torch.device(device)
        self.allow = False
        self.saved = {}
        self.alloc0 = None
        self.log: list[str] = []

    def _alloc_counts(self):
        if self.device.type != "cuda":
            return None
        st = self.torch.cuda.memory_stats(self.device)
        return st.get("num_device_alloc", 0), st.get("num_device_free", 0)

    def arm(self) -> "LaunchWindow":
        """Before the phase (and its timer): the allocation counters the check compares against."""
        self.alloc0 = self._alloc_counts() if self.active else None
        return self

    def check(self) -> None:
        """After the phase (and its timer): no device allocation or free happened in between."""
        if self.alloc0 is None:
            return
        a1 = self._alloc_counts()
        if a1 != self.alloc0:
            raise RuntimeError(f"device memory allocated or freed inside a pending persistent PLL launch "
                               f"(hipMalloc/hipFree counts {self.alloc0} -> {a1})")

    def __enter__(self):
        if not self.active:
            return self
        self.log.append("open")
        if self.dist.is_available() and self.dist.is_initialized():
            for name in _DIST_CALLS:
                fn = getattr(self.dist, name, None)
                if fn is None:
                    continue
                self.saved[name] = fn

                def guarded(*a, _fn=fn, _name=name, **k):
                    if not self.allow:
                        raise RuntimeError(f"torch.distributed.{_name} inside a pending persistent PLL launch "
                                           "(only the per-step gather may run there)")
                    return _fn(*a, **k)
                setattr(self.dist, name, guarded)
        return self

    def __exit__(self, et, ev, tb):
        if not self.active:
            return False
        for name, fn in self.saved.items():
            setattr(self.dist, name, fn)
        self.saved = {}
        self.log.append("close")
        return False

    def gather(self, fn):
        """The per-step gather, the one collective allowed inside the window."""
        if fn is None:
            return None

        def g(**tensors):
            self.allow = True
            try:
                self.log.append("gather")
                return fn(**tensors)
            finally:
                self.allow = False
        return g


def run_rank(args, world: int, rank: int, local: int, stepper_factory=None, backend: str = "nccl") -> dict | None:
    """One rank of the benchmark: its own channel shard, W warm-up + K timed block-steps bracketed
    by barrier + synchronize, max over ranks, gather of each block-step's audio and RDS bits to
    rank 0 (world > 1). Returns the result dict on rank 0 (None elsewhere)."""
    import torch
    import torch.distributed as dist

    if world > 1:
        if backend == "nccl":
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    pkg = _load_pkg()
    from real_time_sdr_amd.sharding import BlockGather, channel_range, max_over_ranks
    first, nch = channel_range(args.channels, rank)
    nblocks = args.warmup + args.steps
    factory = stepper_factory or GpuStepper
    st = factory(args, nch, first, local, nblocks)
    gdev = st.dev if hasattr(st, "dev") else "cpu"
    bg = None
    if world > 1 and not args.no_gather:
        bg = BlockGather(torch, dist, world, st.outputs_spec(), gdev, dst=0)
    gather = bg.gather if bg is not None else None
    pending = bool(getattr(st, "launch_pending", False))
    win_dev = gdev if world == 1 or backend == "nccl" else "cpu"
    try:
        # RCCL connects lazily at a communicator's first collective: one untimed gather round (and
        # the receiving rank's capture buffers) before any phase's persistent launch is pending
        if gather is not None and hasattr(st, "prime_gather"):
            st.prime_gather(gather)
        st.synchronize()
        if world > 1:
            dist.barrier()
        with LaunchWindow(torch, dist, win_dev, pending).arm() as win:
            if hasattr(st, "begin_phase") and args.warmup:
                st.begin_phase(args.warmup)
            for b in range(args.warmup):
                st.step(b, win.gather(gather))
            st.synchronize()
        win.check()
        if world > 1:
            dist.barrier()
        if hasattr(st, "prepare_phase"):
            st.prepare_phase(args.steps)
        win = LaunchWindow(torch, dist, win_dev, pending).arm()
        st.synchronize()
        if os.environ.get("SDR_BENCH_IDLE_MS"):   # diagnosis: the GPU idle before the timer (profiles/r06/idle_gap)
            time.sleep(float(os.environ["SDR_BENCH_IDLE_MS"]) / 1e3)
        t0 = time.perf_counter()
        with win:
            if hasattr(st, "begin_phase"):
                st.begin_phase(args.steps)
            for b in range(args.warmup, nblocks):
                st.step(b, win.gather(gather))
            t_enq = time.perf_counter() - t0          # host time to enqueue the K block-steps
            st.synchronize()
        if world > 1:
            dist.barrier()
        st.synchronize()
        elapsed = time.perf_counter() - t0
        win.check()
        if world > 1:
            elapsed = max_over_ranks(torch, dist, elapsed, gdev)
        # ---- outside the timed region. --dump-outputs: the last timed step's outputs (rank 0's shard)
        dump = getattr(args, "dump_outputs", None)
        if dump and rank == 0 and hasattr(st, "last_outputs"):
            write_outputs(dump, st.last_outputs())
        # everything below the result line's own figures runs with --full only.
        # Parity of the outputs (every rank checks its own captured channels against the oracle; the
        # receiving rank checks that the rows the gather delivered from each rank are the rows that
        # rank produced)
        full = bool(getattr(args, "full", False))
        cpu_legs = full and not args.no_cpu_baseline
        cap = st.captured() if (cpu_legs and hasattr(st, "captured")) else None
        ver = verify_captured(cap, _cpu_share() if world == 1 else max(1, _cpu_share() // 2)) if cap else None
        gathered_check = None
        if world > 1 and cap is not None:
            mine = {"rank": rank, "ok": (ver or {}).get("ok"), "digest": cap["digest"],
                    "channels": [cap["first_channel"] + c for c in cap["channels"]],
                    "mismatches": (ver or {}).get("mismatches")}
            objs = [None] * world if rank == 0 else None
            dist.gather_object(mine, objs, dst=0)
            if rank == 0:
                got = st.gathered_digests() if (bg is not None and hasattr(st, "gathered_digests")) else None
                gathered_check = {
                    "ranks_oracle_ok": all(o["ok"] for o in objs),
                    "channels": {o["rank"]: o["channels"] for o in objs},
                    "mismatches": {o["rank"]: o["mismatches"] for o in objs if o["mismatches"]} or None,
                    "gather_rows_equal": (None if got is None else
                                          all(got[o["rank"]] == o["digest"] for o in objs)),
                }
        res = None
        if rank == 0:
            total_samples = world * nch * st.info.block_iq * args.steps
            res = {
                "metric": METRIC,
                "value": round(total_samples / elapsed / 1e6, 2),
                "unit": "MS/s",
                "n_gpus": world,
                "steps": args.steps,
                "warmup": args.warmup,
                "full": full,
                "ms_per_step": round(elapsed / args.steps * 1e3, 4),
                "host_enqueue_ms_per_step": round(t_enq / args.steps * 1e3, 4),
                "higher_is_better": True,
                "scaling": "weak",
                "vs_baseline": None,
                "dtype": "f32",
                "data": "synthetic FM multiplex I/Q (mono+pilot+stereo+RDS 0A), u8, generated on the device, "
                        "every channel distinct, resident in HBM",
                "config": {
                    "workload": "BASELINE configs[4] per GPU: full mono+stereo+RDS pipeline (project 0 r + mono), "
                                f"{nch} channels/GPU, mode 0 (2.4 MS/s, 73500 I/Q per block)",
                    "channels_per_gpu": nch, "channels_total": world * nch, "distinct_channels": world * nch,
                    "block_iq": st.info.block_iq, "mode": 0,
                    "pll_cus": (f"PLL stream on CU-mask {st.cu_spec}, other streams on the rest"
                                if getattr(st, "cu_spec", "") not in ("", "0", None) else "no CU masks"),
                    "numerics": ("fast: int8 MFMA front end, fm_demod within 1e-5 of the reference, RDS bits "
                                 "bit-exact" if args.numerics == "fast" else "exact (bit-exact with the reference)"),
                    "parallelism": f"channel-sharded x{world}" + (
                        "" if world == 1 or args.no_gather else " + RCCL gather of audio and RDS bits to rank 0"),
                },
            }
            res.update(st.report(args.warmup, elapsed, args.steps))
            if bg is not None:
                res["gathered"] = bg.check_last(world)
            if full and not args.no_isolated and hasattr(st, "isolated_frontend"):
                iso = st.isolated_frontend()
                res["frontend_isolated"] = iso
                res["roofline"]["copy_GBps"] = iso["hbm_copy"]["achieved"]
                res["roofline"]["frac_of_copy"] = round(res["roofline"]["achieved"] / iso["hbm_copy"]["achieved"], 4)
                res["roofline_fast"] = iso.get("fast")
            res["cpu_baseline"] = (cpu_baseline_leg(args, None, timing=(world == 1 and getattr(args, "cpu_timing", True)))
                                   if cpu_legs else None)
            # the queue-plumbed program on the same input (N = 1, outside the timed region)
            if (world == 1 and cpu_legs and hasattr(st, "captured") and
                    os.environ.get("SDR_BENCH_QUEUE", "1") != "0"):
                res["queue_plumbed"] = qp = queue_plumbed_leg(args, st, nch)
                if "value" in qp:
                    qp["vs_value"] = round(qp["value"] / res["value"], 4)
            if ver is not None:
                res["cpu_baseline"]["verified"] = ver
            if gathered_check is not None:
                res["verified_ranks"] = gathered_check
                rows_ok = gathered_check["gather_rows_equal"] if bg is not None else True
                res["verified"] = bool(gathered_check["ranks_oracle_ok"] and rows_ok)
            else:
                res["verified"] = (ver or {}).get("ok")
        return res
    finally:
        if hasattr(st, "close"):
            st.close()
        if world > 1:
            dist.destroy_process_group()


# ------------------------------------------------------------------------------ CPU baseline leg
def _cpu_share() -> int:
    """Host cores this run may use: the affinity mask, capped by SDR_BENCH_CPU_CORES (default 16,
    one GPU's share of the GPU box; nproc there shows the whole machine)."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    return max(1, min(n, int(os.environ.get("SDR_BENCH_CPU_CORES", "16"))))


def _cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _blob(channel: int, nblocks: int) -> bytes:
    synth = _synth_module()
    src = synth.FMMultiplexSource(channel)
    return b"".join(src.next_block().tobytes() for _ in range(nblocks))


def _run_reference(exe, blob: bytes, reps: int, keep: bool = False):
    """Pipe `reps` copies of blob through `<exe> 0 r`; returns the wall seconds (and, with keep, the
    program's stdout: its PCM)."""
    with tempfile.TemporaryFile() as out:
        t0 = time.perf_counter()
        p = subprocess.Popen([str(exe), "0", "r"], stdin=subprocess.PIPE, stdout=out, stderr=subprocess.DEVNULL)
        try:
            for _ in range(reps):
                p.stdin.write(blob)
            p.stdin.close()
        except BrokenPipeError:
            pass
        p.wait()
        dt = time.perf_counter() - t0
        if not keep:
            return dt
        out.seek(0)
        return dt, out.read()


def _dropin_leg(gpu_exe, blob: bytes, reps: int, nblk: int, dt_ref: float, pcm_ref: bytes) -> dict:
    """The unchanged program on the GPU: the reference's own src/project.cpp linked against
    libsdr_host.so (oracle/_ref/project_gpu: its three stage threads over the C ABI, one channel),
    `project_gpu 0 r` on the same stdin as the reference's `project 0 r`, timed beside it; its PCM is
    compared with the reference program's over their common length (both end by exit(1) on EOF,
    rffrontend.cpp:50-52, which can cut the last blocks of either)."""
    synth = _synth_module()
    dt, pcm = _run_reference(gpu_exe, blob, reps, keep=True)
    n = min(len(pcm), len(pcm_ref))
    per_block = 2 * 2 * synth.BLOCK_IQ // 50          # stereo int16 frames of one block (2940 x 2 B)
    samples = reps * nblk * synth.BLOCK_IQ
    rt = samples / 2.4e6                               # the input's duration at 2.4 MS/s
    return {"value": round(samples / dt / 1e6, 3), "unit": "MS/s", "kind": "dropin",
            "real_time_factor": round(rt / dt, 1), "wall_s": round(dt, 3),
            "reference_value": round(samples / dt_ref / 1e6, 3), "reference_wall_s": round(dt_ref, 3),
            "speedup_vs_reference": round(dt_ref / dt, 3),
            "pcm_equal_blocks": n // per_block if pcm[:n] == pcm_ref[:n] else -1,
            "blocks": reps * nblk,
            "sample": f"the reference's unmodified src/project.cpp linked against libsdr_host.so "
                      f"(oracle/_ref/project_gpu 0 r: 3 stage threads, 1 channel on the GPU) on the same "
                      f"{reps * nblk} blocks via stdin as the reference `project 0 r` run beside it"}


def _check_channel(job):
    """Oracle run of one captured channel (the checker; runs in a worker process)."""
    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle
    j, iq, mono, lr, bits, nbits = job
    ref = oracle.run_channel(iq, 0, True)
    bad = []
    for b in range(iq.shape[0]):
        if not np.array_equal(mono[b], ref["mono"][b]):
            bad.append(f"mono b{b}")
        if not np.array_equal(lr[b], ref["stereo"][b]):
            bad.append(f"stereo b{b}")
        rb = ref["bits"][b]
        if rb is None:
            if int(nbits[b]) != -1:
                bad.append(f"nbits b{b}")
        elif int(nbits[b]) != len(rb) or not np.array_equal(bits[b][:len(rb)], rb.astype(np.uint8)):
            bad.append(f"bits b{b}")
    return j, bad[:4]


def _host_cpus() -> dict:
    """What this process may run on: nproc, the affinity mask, and the cgroup CPU quota if any."""
    out = {"nproc": os.cpu_count()}
    try:
        out["affinity"] = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        out["affinity"] = os.cpu_count()
    quota = None
    try:   # cgroup v2: "max 100000" or "<quota> <period>"
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(p)
    except (OSError, ValueError):
        pass
    out["cgroup_cpu_quota"] = quota
    usable = out["affinity"] or 1
    if quota is not None:
        usable = min(usable, int(quota))
    out["usable"] = max(1, usable)
    return out


def _reference_concurrent(exe, nproc: int, nb: int, reps: int) -> tuple[float, float]:
    """nproc concurrent `project 0 r` processes (3 threads each, the reference's topology) on distinct
    channels, each piping reps x nb blocks; returns (MS/s aggregate, wall seconds)."""
    synth = _synth_module()
    distinct = min(nproc, 16)          # channel content does not change the CPU cost; 16 distinct inputs
    blobs = [_blob(1 + i, nb) for i in range(distinct)]
    with cf.ThreadPoolExecutor(nproc) as ex:
        t0 = time.perf_counter()
        list(ex.map(lambda i: _run_reference(exe, blobs[i % distinct], reps), range(nproc)))
        dt = time.perf_counter() - t0
    return nproc * reps * nb * synth.BLOCK_IQ / dt / 1e6, dt


def verify_captured(cap: dict, workers: int) -> dict:
    """The checker: captured GPU outputs of a few channels (mono, stereo, RDS bits of every block)
    compared bit for bit with the oracle run on the same input bytes (worker processes)."""
    jobs = [(j, cap["iq"][:, j], cap["mono"][:, j], cap["lr"][:, j], cap["bits"][:, j], cap["nbits"][:, j])
            for j in range(len(cap["channels"]))]
    with cf.ProcessPoolExecutor(max(1, min(len(jobs), workers)), mp_context=mp.get_context("spawn")) as ex:
        results = dict(ex.map(_check_channel, jobs))
    first = cap.get("first_channel", 0)
    bad = {first + cap["channels"][j]: v for j, v in results.items() if v}
    return {"ok": not bad, "channels": [first + c for c in cap["channels"]], "blocks": int(cap["iq"].shape[0]),
            "outputs": "mono int16, stereo int16, RDS bits (every block incl. warm-up), "
                       "bit for bit against the oracle on the same input bytes",
            "mismatches": bad or None}


def cpu_baseline_leg(args, cap: dict | None, timing: bool = True) -> dict:
    """Rank 0 only, outside the timed region: (1) the reference's own program (oracle/_ref/project,
    built from the unmodified sources) in its 3-thread topology on one channel; (2) the same
    program on distinct channels concurrently over one GPU's CPU share (floor(cores/3) processes);
    (3) the same over every CPU this job may use on the host (floor(usable/3) processes, the node's
    CPU figure); (4) with `cap`, the checker (verify_captured)."""
    synth = _synth_module()
    exe = ROOT / "oracle" / "_ref" / "project"
    cores = _cpu_share()
    host = _host_cpus()
    res: dict = {"host_cpu": _cpu_model(), "nproc": os.cpu_count(), "cpu_share": cores}
    if not timing:
        # N > 1: the CPU legs are timed at N = 1 only (BASELINE's CPU comparison is per node, and the
        # other ranks have finished); the captured outputs are still checked
        res.update({"value": None, "unit": "MS/s", "cores": 0, "kind": "reference",
                    "sample": "not timed at N > 1 (see the N = 1 line)"})
    elif exe.exists():
        nblk = 32
        blob = _blob(0, nblk)
        reps = 150  # 4800 blocks = 353 M I/Q samples (~10 s at the reference's ~37 MS/s)
        dt, pcm_ref = _run_reference(exe, blob, reps, keep=True)
        res.update({"value": round(reps * nblk * synth.BLOCK_IQ / dt / 1e6, 3), "unit": "MS/s", "cores": 3,
                    "kind": "reference",
                    "sample": f"reference `project 0 r` (src/*.cpp, g++ -O3, 3 threads RF/audio/RDS) on "
                              f"{reps * nblk} blocks = {reps * nblk * synth.BLOCK_IQ / 1e6:.1f} M I/Q samples of "
                              f"1 channel via stdin, {dt:.2f} s wall"})
        gpu_exe = ROOT / "oracle" / "_ref" / "project_gpu"
        if gpu_exe.exists() and os.environ.get("SDR_BENCH_DROPIN", "1") != "0":
            try:
                res["dropin_1ch"] = _dropin_leg(gpu_exe, blob, reps, nblk, dt, pcm_ref)
            except (OSError, subprocess.SubprocessError) as exc:
                res["dropin_1ch"] = {"error": str(exc)}
        nproc = max(1, cores // 3)
        v, dt2 = _reference_concurrent(exe, nproc, 8, 400)     # per process: 3200 blocks of its own channel
        res["all_cores"] = {"value": round(v, 3), "unit": "MS/s", "cores": 3 * nproc, "kind": "reference",
                            "sample": f"{nproc} concurrent `project 0 r` processes x 3 threads, distinct channels, "
                                      f"3200 blocks each, {dt2:.2f} s wall (one GPU's CPU share)"}
        res["host_cpus"] = host
        # the node's CPU figure by extrapolation (not measured: this job's cgroup owns `usable` CPUs):
        # the measured rate per reference process times floor(nproc / 3) processes, i.e. the 3-thread
        # topology (project.cpp:134-136) on every hardware thread of the host with perfect scaling
        nproc_node = max(1, (host["nproc"] or 1) // 3)
        res["node_extrapolated"] = {
            "value": round(v / nproc * nproc_node, 3), "unit": "MS/s", "cores": 3 * nproc_node,
            "kind": "reference", "measured": False,
            "sample": f"all_cores rate per process ({v / nproc:.2f} MS/s) x {nproc_node} processes = "
                      f"floor(nproc {host['nproc']} / 3); an upper bound (perfect scaling, no SMT or memory "
                      f"contention) for the whole node's CPUs"}
        # the whole host (floor(usable / 3) processes) only on request: a GPU job on this pool owns a
        # 16-CPU share of the node, the other GPUs' jobs share the rest (SDR_BENCH_CPU_CORES)
        if os.environ.get("SDR_BENCH_HOST_LEG", "0") == "1":
            nproc_h = max(1, host["usable"] // 3)
            v, dt3 = _reference_concurrent(exe, nproc_h, 8, 200)   # 1600 blocks per process
            res["all_host_cores"] = {
                "value": round(v, 3), "unit": "MS/s", "cores": 3 * nproc_h, "kind": "reference",
                "processes": nproc_h, "nproc": host["nproc"], "affinity": host["affinity"],
                "cgroup_cpu_quota": host["cgroup_cpu_quota"],
                "sample": f"{nproc_h} concurrent `project 0 r` processes x 3 threads (floor(usable CPUs / 3); "
                          f"usable = min(affinity {host['affinity']}, cgroup quota {host['cgroup_cpu_quota']}) "
                          f"of nproc {host['nproc']}), 1600 blocks each, {dt3:.2f} s wall"}
    else:
        # the C restatement, one core, full pipeline (this tree built without /root/reference)
        sys.path.insert(0, str(ROOT / "oracle"))
        import oracle
        blocks = np.frombuffer(_blob(0, 8), np.uint8).reshape(8, -1)
        ch = oracle.Channel(0, True)
        t0, n = time.perf_counter(), 0
        while time.perf_counter() - t0 < 8.0:
            fm = ch.frontend(blocks[n % 8])
            ch.mono(fm)
            ch.stereo(fm)
            ch.rds(fm)
            n += 1
        dt = time.perf_counter() - t0
        res.update({"value": round(n * synth.BLOCK_IQ / dt / 1e6, 3), "unit": "MS/s", "cores": 1, "kind": "port",
                    "sample": f"oracle C restatement, 1 channel x {n} blocks, 1 thread, {dt:.2f} s"})
    if cap is not None:
        res["verified"] = verify_captured(cap, cores)
    return res


# ------------------------------------------------------------------ the queue-plumbed program
def _multi_structs():
    """ctypes mirrors of include/sdr_multi.h (sdr_multi_opts, sdr_multi_stats)."""
    import ctypes as C

    class Opts(C.Structure):
        _fields_ = [("nch", C.c_int), ("mode", C.c_int), ("flags", C.c_int), ("device", C.c_int),
                    ("pll_cus", C.c_int), ("in_path", C.c_char_p), ("d_iq", C.c_void_p),
                    ("row_stride", C.c_size_t), ("block_stride", C.c_size_t), ("nblocks", C.c_int),
                    ("out_prefix", C.c_char_p), ("ncap", C.c_int), ("cap_blocks", C.c_int),
                    ("cap_ch", C.POINTER(C.c_int)), ("cap_lr", C.c_void_p), ("cap_nbits", C.c_void_p),
                    ("cap_bits", C.c_void_p), ("stamp_blocks", C.c_int), ("pll_end", C.c_void_p)]

    class Stats(C.Structure):
        _fields_ = [("blocks", C.c_longlong), ("seconds", C.c_double), ("steady_seconds", C.c_double),
                    ("pll_period_ms", C.c_double), ("pll_span_ms", C.c_double), ("read_s", C.c_double),
                    ("h2d_ms", C.c_double),
                    ("d2h_ms", C.c_double), ("persistent", C.c_int)]
    return Opts, Stats


QUEUE_WARM_BLOCKS = 40    # untimed blocks before the queue child's timed run


def queue_child(a) -> None:
    """bench.py --queue-child: the multi-channel receiver engine (include/sdr_multi.h: the reference's
    three stage threads joined by ThreadSafeQueue<FmBatch*>, threadsafequeue.h:24-74) over the bench's
    own device-generated input (the same generator, seed and channels), in a process of its own so a
    failure of the engine cannot take the bench line with it. Writes the captured rows of the checked
    channels to --cap-out and prints one JSON line of the engine's timings."""
    import ctypes as C
    import torch
    pkg = _load_pkg()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    iq = make_input(torch, a.channels, a.blocks, first_channel=0, device=dev)
    host = C.CDLL(str(ROOT / "real-time-sdr_amd" / "libsdr_host.so"))
    Opts, Stats = _multi_structs()
    host.sdr_multi_run.argtypes = [C.POINTER(Opts), C.POINTER(Stats)]
    host.sdr_multi_run.restype = C.c_int
    info = pkg.Pipeline(1).info
    ch = [int(c) for c in a.cap_ch.split(",")]
    nb, nv = a.blocks, len(ch)
    lr = np.zeros((nb, nv, 2 * info.n_audio), np.int16)
    nbits = np.zeros((nb, nv), np.int32)
    bits = np.zeros((nb, nv, pkg.SDR_MAX_BITS), np.uint8)
    cap_ch = (C.c_int * nv)(*ch)
    ends = np.zeros((2, nb), np.uint64)

    lr2, nbits2, bits2 = np.zeros_like(lr), np.zeros_like(nbits), np.zeros_like(bits)

    def run(cap) -> "Stats":
        c_lr, c_nbits, c_bits = cap
        o = Opts(nch=a.channels, mode=0, flags=0, device=0, pll_cus=a.cus, in_path=None, d_iq=iq.data_ptr(),
                 row_stride=iq.stride(1), block_stride=iq.stride(0), nblocks=nb, out_prefix=None,
                 ncap=nv, cap_blocks=nb, cap_ch=cap_ch, cap_lr=c_lr.ctypes.data,
                 cap_nbits=c_nbits.ctypes.data, cap_bits=c_bits.ctypes.data,
                 stamp_blocks=nb, pll_end=ends.ctypes.data)
        st = Stats()
        torch.cuda.synchronize(dev)
        rc = host.sdr_multi_run(C.byref(o), C.byref(st))
        if rc != 0:
            raise SystemExit(f"sdr_multi_run: {rc} {pkg.lib().sdr_last_error()}")
        return st
    # run 1 (untimed, like the bench's warm-up): the checked captures, and the process's first use of
    # every kernel and buffer; more untimed runs up to 40 warm-up blocks in all (bench.py's default
    # warm-up; the child starts on a GPU idle since the bench's CPU legs); the timed run: the same
    # blocks from the initial state again (the engine's pooled contexts, reset), its captures compared
    # with run 1's
    run((lr, nbits, bits))
    for _ in range(1, -(-QUEUE_WARM_BLOCKS // nb)):
        run((lr2, nbits2, bits2))
    t_call = time.perf_counter()
    st = run((lr2, nbits2, bits2))
    call_s = time.perf_counter() - t_call          # the timed run's call: set-up + run + tear-down
    timed_equal = bool(np.array_equal(lr, lr2) and np.array_equal(nbits, nbits2))
    for b, j in np.argwhere(nbits > 0) if timed_equal else ():        # the bits a row holds
        k = int(nbits[b, j])
        timed_equal = timed_equal and np.array_equal(bits[b, j, :k], bits2[b, j, :k])
    if not timed_equal:
        print(f"queue child: timed run differs: lr {np.array_equal(lr, lr2)} nbits {np.array_equal(nbits, nbits2)}",
              file=sys.stderr)
    period_us = [[round(float(e[b] - e[b - 1]) / 100.0, 1) for b in range(1, nb)] for e in ends]
    np.savez(a.cap_out, lr=lr, nbits=nbits, bits=bits)
    import hashlib
    iq_sha = hashlib.sha256(np.ascontiguousarray(iq[:, ch].cpu().numpy()).tobytes()).hexdigest()
    print(json.dumps({"iq_sha": iq_sha, "pll_block_us": period_us, "blocks": st.blocks, "seconds": st.seconds, "steady_seconds": st.steady_seconds,
                      "pll_period_ms": st.pll_period_ms, "pll_span_ms": st.pll_span_ms, "d2h_ms": st.d2h_ms, "persistent": st.persistent,
                      "call_s": call_s, "timed_run_equal": timed_equal,
                      "block_iq": info.block_iq}), flush=True)


def queue_plumbed_leg(args, st, nch: int) -> dict:
    """Rank 0 at N = 1, outside the timed region: the same channels and blocks through the
    queue-plumbed receiver (queue_child), its rate next to `value`, and its captured stereo audio and
    RDS bits compared with the bench's own captures of the same channels (which the checker compared
    with the oracle): equal rows mean the queue program is verified against the oracle too."""
    import tempfile
    # the blocks before the bench's input wraps (INPUT_RING): the child regenerates those in order
    nb = st.ring
    cap = {k: (v[:nb] if k in ("iq", "lr", "bits", "nbits") else v) for k, v in st.captured().items()}
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "cap.npz")
        cus = int(st.cu_spec) if str(getattr(st, "cu_spec", "")).isdigit() else 64
        cmd = [sys.executable, str(pathlib.Path(__file__).resolve()), "--queue-child", "--channels", str(nch),
               "--blocks", str(nb), "--cus", str(cus), "--cap-ch", ",".join(str(c) for c in cap["channels"]),
               "--cap-out", out]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        except subprocess.SubprocessError as exc:
            return {"error": str(exc)}
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            return {"error": f"exit {r.returncode}: {r.stderr[-500:]}"}
        q = json.loads(lines[-1])
        import hashlib
        if q["iq_sha"] != hashlib.sha256(np.ascontiguousarray(cap["iq"]).tobytes()).hexdigest():
            return {"error": "the child's regenerated input differs from the bench's"}
        got = np.load(out)
        equal = np.array_equal(got["lr"], cap["lr"]) and np.array_equal(got["nbits"], cap["nbits"])
        for b, j in np.argwhere(cap["nbits"] > 0) if equal else ():   # the bits a row holds
            k = int(cap["nbits"][b, j])
            equal = equal and np.array_equal(got["bits"][b, j, :k], cap["bits"][b, j, :k])
    samples = nch * q["block_iq"]
    res = {
        "program": "real-time-sdr_amd/host/sdr_multi_engine.cpp (include/sdr_multi.h): RF / audio / RDS threads "
                   "(project.cpp:134-136), ThreadSafeQueue<FmBatch*> (threadsafequeue.h:24-74) with device-resident "
                   "fm_demod batches, one context per thread, each consumer's PLL as its own persistent launch "
                   "(sdr_plls_launch_sel), L/R PCM and RDS bits copied to the host every block",
        "input": f"the bench's device-generated input, same channels and blocks ({q['blocks']} blocks incl. the "
                 f"warm-up), regenerated in a child process; timed: a run over those blocks after untimed runs of "
                 f">= {QUEUE_WARM_BLOCKS} blocks in all (the first gives the checked captures), from the "
                 f"initial state (pooled contexts reset), its outputs equal to the first run's",
        "value": round(q["blocks"] * samples / q["seconds"] / 1e6, 2), "unit": "MS/s",
        "ms_per_block": round(q["seconds"] / q["blocks"] * 1e3, 4),
        "pll_period_value": (round(samples / (q["pll_period_ms"] * 1e-3) / 1e6, 2) if q["pll_period_ms"] else None),
        "pll_period_ms": round(q["pll_period_ms"], 4),
        "outside_pll_span_ms": round(q["seconds"] * 1e3 - q["pll_span_ms"], 3),
        "pll": "persistent" if q["persistent"] else "per-block dispatch",
        "d2h_ms": round(q["d2h_ms"], 2),
        "outputs_equal_to_bench_capture": bool(equal),
        "timed_run_outputs_equal": q.get("timed_run_equal"),
        "checked_channels": cap["channels"],
    }
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    # 40 untimed blocks (~30 ms): the shader clock settles from ~2316 to ~2380 MHz under the sustained
    # load only after tens of ms, so a 5-block warm-up times the clock ramp, not the steady state
    # (profiles/r04/warmup_ab.txt: 20 steps 0.720 ms after 5 warm-up blocks, 0.700-0.702 after 40)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--channels", type=int, default=1024, help="channels per GPU")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also: the oracle check of the captured channels, the CPU "
                         "baselines, the isolated front-end and copy timings, the queue-plumbed receiver")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (rank 0's channels) as DIR/<name>.npy, float32")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the CPU legs, the oracle check and the queue-plumbed receiver")
    ap.add_argument("--no-gather", action="store_true", help="skip the per-step RCCL gather (N>1)")
    ap.add_argument("--no-isolated", action="store_true", help="with --full: skip the isolated front-end timings")
    ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl", help=argparse.SUPPRESS)
    ap.add_argument("--numerics", choices=("exact", "fast"), default="exact",
                    help="exact: every output bit-identical to the reference; fast: the matrix-core front end "
                         "(fm_demod within 1e-5, RDS bits bit-exact)")
    ap.add_argument("--queue-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--blocks", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--cus", type=int, default=64, help=argparse.SUPPRESS)
    ap.add_argument("--cap-ch", default="0", help=argparse.SUPPRESS)
    ap.add_argument("--cap-out", default="", help=argparse.SUPPRESS)
    argv = sys.argv[1:]
    args = ap.parse_args(argv)
    if args.queue_child:
        queue_child(args)
        return
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args, argv))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"bench: WORLD_SIZE={world} (--gpus {args.gpus}); measuring {world} rank(s)", file=sys.stderr)
    res = run_rank(args, world, rank, local)
    if res is not None:
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
