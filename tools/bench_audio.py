#!/usr/bin/env python3
"""Timing of the audio finishing stage (sdr_audio_finish, sdr_audio_blend_from_meter) in one process,
mode 0, width 2.

  1. The kernel alone, by HIP events around `iters` back-to-back calls on one stream after a warm-up,
     interleaved over `repeat` rounds; each call reads and writes another of `ring` row buffers (24 x
     2 x 6 MB at 1024 channels: more than the last-level cache holds):
       sdr_audio_finish shape 0-3     32 channels x 64 frames, 16 x 128, 8 x 128, 4 x 128 per workgroup
                                      and tile (SDR_AUDIO_SHAPE at create; 2 is the default)
       sdr_hbm_copy                   the same bytes through the calibration copy kernel
     and against the chain floor N * 2 * L / f: N steps of two dependent f32 operations, L = 8.1 cycles
     (the dependent-VALU latency the PLL measured), f = --shader-mhz (2400, the peak engine
     clock; the pipeline bench sustains 2300-2380).
  2. The pipeline step on bench.py's three-stream persistent schedule, metered (tools/bench_meter.py's
     stepper), interleaved: as it is, and with blend_from_meter + finish per block on the post stream.

Prints one JSON line per measurement and writes them to profiles/r10/audio/bench_audio.jsonl (--out).
  python tools/bench_audio.py [--channels 1024] [--iters 200] [--repeat 5] [--steps 100] [--warmup 40]
"""
from __future__ import annotations

import argparse
import json
import os
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import bench  # noqa: E402
import bench_tuner  # noqa: E402
from bench_meter import MeteredStepper  # noqa: E402
from bench_scan import timed  # noqa: E402

WARM = 40
SHAPES = {0: "32ch x 64", 1: "16ch x 128", 2: "8ch x 128", 3: "4ch x 128"}
CHAIN_LATENCY = 8.1     # cycles per dependent VALU operation of a lone wave


def kernel_alone(torch, pkg, nch: int, iters: int, repeat: int, ring: int, mhz: float, emit) -> None:
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    n = pkg.Pipeline(1).info.n_audio
    nbytes = nch * 2 * n * 2
    src = torch.randint(-32768, 32768, (ring, nch, 2 * n), dtype=torch.int16, device=dev)
    dst = torch.empty_like(src)
    fins = {}
    for shape in SHAPES:
        os.environ["SDR_AUDIO_SHAPE"] = str(shape)
        fins[shape] = pkg.AudioFinish(nch)
    del os.environ["SDR_AUDIO_SHAPE"]
    legs = {f"sdr_audio_finish_shape{k}": (lambda b, f=f: f.finish(src[b % ring], out=dst[b % ring], stream=s))
            for k, f in fins.items()}
    legs["sdr_hbm_copy"] = lambda b: pkg.hbm_copy(dst[b % ring].view(torch.uint8).reshape(-1),
                                                  src[b % ring].view(torch.uint8).reshape(-1), stream=s)
    got: dict = {k: [] for k in legs}
    for call in legs.values():
        for b in range(WARM):
            call(b)
    torch.cuda.synchronize(dev)
    for rep in range(repeat):
        for name, call in legs.items():
            ms = timed(torch, s, call, iters)
            got[name].append(ms)
            emit({"leg": "kernel_alone", "call": name, "repeat": rep, "channels": nch, "iters": iters, "ring": ring,
                  "ms_per_call": round(ms, 4), "MB_read": round(nbytes / 1e6, 2), "GBps_read_plus_written": round(2 * nbytes / ms / 1e6, 1)})
    med = {k: statistics.median(v) for k, v in got.items()}
    floor_ms = n * 2 * CHAIN_LATENCY / (mhz * 1e3)
    best = min((k for k in med if k != "sdr_hbm_copy"), key=lambda k: med[k])
    emit({"leg": "kernel_alone_summary", "channels": nch, "shapes": SHAPES,
          "median_ms": {k: round(v, 4) for k, v in med.items()},
          "min_ms": {k: round(min(v), 4) for k, v in got.items()}, "max_ms": {k: round(max(v), 4) for k, v in got.items()},
          "best": best, "default_shape_over_copy": round(med["sdr_audio_finish_shape2"] / med["sdr_hbm_copy"], 2),
          "best_over_copy": round(med[best] / med["sdr_hbm_copy"], 2),
          "shader_MHz": mhz, "chain_floor_ms": round(floor_ms, 4),
          "default_shape_over_chain_floor": round(med["sdr_audio_finish_shape2"] / floor_ms, 2),
          "best_over_chain_floor": round(med[best] / floor_ms, 2)})
    torch.cuda.synchronize(dev)
    for f in fins.values():
        f.close()


class FinishedStepper(MeteredStepper):
    """The metered stepper plus blend_from_meter and finish of every block on the post stream, into rows
    of the stage's own."""

    def __init__(self, args, nch, first, local, nblocks):
        super().__init__(args, nch, first, local, nblocks)
        self.fin = self.pkg.AudioFinish(nch, device=local)
        self.fin_out = [self.torch.empty_like(self.lr[0]) for _ in range(2)]

    def step(self, b, gather=None):
        super().step(b, gather)
        s = self.s_post
        self.fin.blend_from_meter(self.meter, stream=s)
        self.fin.finish(self.lr[b % 2], out=self.fin_out[b % 2], stream=s)
        self.post_done[b].record(s)

    def close(self):
        self.torch.cuda.synchronize(self.dev)
        self.fin.close()
        super().close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--ring", type=int, default=24, help="row buffers the calls alone rotate over")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=5, help="interleaved repeats of every leg")
    ap.add_argument("--shader-mhz", type=float, default=2400.0, help="f of the chain floor")
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r10" / "audio"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_audio: needs a GPU")
    pkg = bench._load_pkg()
    out = pathlib.Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    lines = []

    def emit(d: dict) -> None:
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        (out / "bench_audio.jsonl").write_text("\n".join(lines) + "\n")

    if not args.skip_calls:
        kernel_alone(torch, pkg, args.channels, args.iters, args.repeat, args.ring, args.shader_mhz, emit)
        torch.cuda.empty_cache()
    if not args.skip_pipeline:
        legs = (("metered", MeteredStepper), ("finished", FinishedStepper))
        got: dict = {n: [] for n, _ in legs}
        for rep in range(min(args.repeat, 3)):
            for name, factory in legs:
                r = bench_tuner.pipeline_step(args, factory, "4")
                got[name].append(r["ms_per_step"])
                emit({"leg": "pipeline_step", "name": name, "repeat": rep, "channels": args.channels, **r})
        med = {n: statistics.median(v) for n, v in got.items()}
        emit({"leg": "pipeline_ratio", "median_ms": med,
              "spread_ms": {n: [min(v), max(v)] for n, v in got.items()},
              "finished_over_metered": round(med["finished"] / med["metered"], 4)})


if __name__ == "__main__":
    main()
