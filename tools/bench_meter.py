#!/usr/bin/env python3
"""Timing of the reception meter (sdr_meter_audio, sdr_meter_rds) in one process, mode 0.

  1. Calls alone, by HIP events around `iters` back-to-back calls on one stream after a warm-up,
     interleaved over `repeat` rounds. Each call reads the rows of another of `ring` resident contexts
     (4 x 66.6 MB at 1024 channels: more than the last-level cache holds), every context one block in:
       sdr_meter_audio          fm + history, pilot and the L/R PCM of every channel
       sdr_meter_rds            rds_band and rds_clean of every channel
       sdr_hbm_copy             the bytes each call reads through the calibration copy kernel: the byte
                                floor (the copy also writes them, the meter writes 64 bytes a channel)
     and each call as a ratio to its copy.
  2. The pipeline step on bench.py's three-stream persistent schedule (bench.run_rank with the bench's
     warm-up), interleaved: as the bench runs it, and with both meter calls per block on the post
     stream. The claim under test: the metered step stays within the run-to-run spread of the unmetered
     one (the step is PLL-bound and the meter runs on the other CUs).

Prints one JSON line per measurement and writes them to profiles/r09/meter/bench_meter.jsonl (--out).
  python tools/bench_meter.py [--channels 1024] [--iters 200] [--repeat 5] [--steps 100] [--warmup 40]
"""
from __future__ import annotations

import argparse
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import bench  # noqa: E402
import bench_tuner  # noqa: E402
from bench_scan import timed  # noqa: E402

WARM = 40


def calls_alone(torch, pkg, iq, nch: int, iters: int, repeat: int, ring: int, emit) -> None:
    dev = iq.device
    s = torch.cuda.Stream(dev)
    pipes, lrs = [], []
    for r in range(ring):                      # one block through every context: its rows are the calls' input
        pipe = pkg.Pipeline(nch)
        with torch.cuda.stream(s):
            pipe.frontend(iq[r % iq.shape[0]], stream=s)
            lrs.append(pipe.stereo(stream=s))
            pipe.rds(stream=s)
        pipes.append(pipe)
    meter = pkg.Meter(nch)
    info = pipes[0].info
    b_audio = nch * (4 * (info.block_if + 100) + 4 * info.block_if + 2 * 2 * info.n_audio)
    b_rds = nch * (4 * info.block_if + 4 * info.n_rds)
    bufs = {}
    for name, nbytes in (("audio", b_audio), ("rds", b_rds)):
        n16 = (nbytes + 15) // 16 * 16
        bufs[name] = (torch.empty(ring, n16, dtype=torch.uint8, device=dev), torch.empty(n16, dtype=torch.uint8, device=dev))
    legs = {
        "sdr_meter_audio": lambda b: meter.audio(pipes[b % ring], lrs[b % ring], stream=s),
        "sdr_meter_rds": lambda b: meter.rds(pipes[b % ring], stream=s),
        "sdr_hbm_copy_audio_bytes": lambda b: pkg.hbm_copy(bufs["audio"][1], bufs["audio"][0][b % ring], stream=s),
        "sdr_hbm_copy_rds_bytes": lambda b: pkg.hbm_copy(bufs["rds"][1], bufs["rds"][0][b % ring], stream=s),
    }
    read = {"sdr_meter_audio": b_audio, "sdr_meter_rds": b_rds, "sdr_hbm_copy_audio_bytes": b_audio,
            "sdr_hbm_copy_rds_bytes": b_rds}
    got: dict = {k: [] for k in legs}
    for call in legs.values():
        for b in range(WARM):
            call(b)
    torch.cuda.synchronize(dev)
    for rep in range(repeat):
        for name, call in legs.items():
            ms = timed(torch, s, call, iters)
            got[name].append(ms)
            emit({"leg": "call_alone", "call": name, "repeat": rep, "channels": nch, "iters": iters, "ring": ring,
                  "ms_per_call": round(ms, 4), "read_MB": round(read[name] / 1e6, 1),
                  "GBps_read": round(read[name] / ms / 1e6, 1)})
    med = {k: statistics.median(v) for k, v in got.items()}
    emit({"leg": "call_alone_summary", "channels": nch, "median_ms": {k: round(v, 4) for k, v in med.items()},
          "min_ms": {k: round(min(v), 4) for k, v in got.items()},
          "max_ms": {k: round(max(v), 4) for k, v in got.items()},
          "read_MB": {"audio": round(b_audio / 1e6, 1), "rds": round(b_rds / 1e6, 1)},
          "audio_over_copy": round(med["sdr_meter_audio"] / med["sdr_hbm_copy_audio_bytes"], 2),
          "rds_over_copy": round(med["sdr_meter_rds"] / med["sdr_hbm_copy_rds_bytes"], 2),
          "noise_fir_GFLOP": round(nch * (info.block_if // 5) * 101 * 2 / 1e9, 3)})
    torch.cuda.synchronize(dev)
    meter.close()
    for pipe in pipes:
        pipe.close()


class MeteredStepper(bench.GpuStepper):
    """The bench's stepper plus both meter calls of every block on the post stream, after the block's
    post stages; the block's post_done event then covers them, so whatever waited for the block's
    outputs also waits for its readings."""

    def __init__(self, args, nch, first, local, nblocks):
        super().__init__(args, nch, first, local, nblocks)
        self.meter = self.pkg.Meter(nch, device=local)

    def step(self, b, gather=None):
        super().step(b, gather)
        s = self.s_post
        s.wait_event(self.post_done[b])
        self.meter.audio(self.pipe, self.lr[b % 2], stream=s)
        self.meter.rds(self.pipe, stream=s)
        self.post_done[b].record(s)

    def close(self):
        self.torch.cuda.synchronize(self.dev)
        self.meter.close()
        super().close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--ring", type=int, default=4, help="resident contexts the calls alone rotate over")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=5, help="interleaved repeats of every leg")
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r09" / "meter"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_meter: needs a GPU")
    pkg = bench._load_pkg()
    dev = torch.device("cuda", 0)
    out = pathlib.Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    lines = []

    def emit(d: dict) -> None:
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        (out / "bench_meter.jsonl").write_text("\n".join(lines) + "\n")

    if not args.skip_calls:
        iq = bench.make_input(torch, args.channels, args.ring, 0, dev)
        calls_alone(torch, pkg, iq, args.channels, args.iters, args.repeat, args.ring, emit)
        del iq
        torch.cuda.empty_cache()
    if not args.skip_pipeline:
        legs = (("unmetered", None), ("metered", MeteredStepper))
        got: dict = {n: [] for n, _ in legs}
        for rep in range(min(args.repeat, 3)):
            for name, factory in legs:
                r = bench_tuner.pipeline_step(args, factory, "4")
                got[name].append(r["ms_per_step"])
                emit({"leg": "pipeline_step", "name": name, "repeat": rep, "channels": args.channels, **r})
        med = {n: statistics.median(v) for n, v in got.items()}
        emit({"leg": "pipeline_ratio", "median_ms": med,
              "spread_ms": {n: [min(v), max(v)] for n, v in got.items()},
              "metered_over_unmetered": round(med["metered"] / med["unmetered"], 4)})


if __name__ == "__main__":
    main()
