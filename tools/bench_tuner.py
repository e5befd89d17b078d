#!/usr/bin/env python3
"""Timing of the shared-capture tuner (sdr_frontend_tuned) against the untuned path, in one process.

  1. The tuned kernel alone, by its workgroup stamps (sdr_frontend_timing): 1024 channels on 128
     source rows (8 stations per row) and on 1024 rows (one station per row), against k_frontend2
     at 1024 channels. Each launch reads another resident input block.
  2. The full pipeline step on bench.py's three-stream persistent schedule (bench.run_rank with the
     bench's warm-up), with sdr_frontend_tuned in place of sdr_frontend, against the untuned step.
     A tuned context has no pipeline fill by parts, so the untuned step is measured both as the bench
     runs it (first block in 4 parts) and with SDR_BENCH_FILL_PARTS=1, the like-for-like figure.

Prints one JSON line per measurement and writes them to profiles/r07/tuner/ (--out).
  python tools/bench_tuner.py [--channels 1024] [--rows 128] [--steps 100] [--warmup 40] [--repeat 3]
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
import bench  # noqa: E402

OFFSETS = (0, -1199, 1200, -600, 500, -37, 901, 250)


def tuning(nch: int, nsrc: int):
    """Channel c on row c % nsrc; the stations of a row get different offsets."""
    return [c % nsrc for c in range(nch)], [OFFSETS[(c // nsrc) % len(OFFSETS)] for c in range(nch)]


def kernel_alone(torch, pkg, iq, nch: int, nsrc: int | None, iters: int) -> dict:
    dev = iq.device
    pipe = pkg.Pipeline(nch)
    if nsrc:
        pipe.set_tuning(*tuning(nch, nsrc), nsrc)
    s = torch.cuda.Stream(dev)
    run = (lambda b: pipe.frontend_tuned(iq[b % iq.shape[0], :nsrc], stream=s)) if nsrc else \
          (lambda b: pipe.frontend(iq[b % iq.shape[0]], stream=s))
    for b in range(40):                       # the bench's warm-up
        run(b)
    torch.cuda.synchronize(dev)
    pipe.frontend_timing(iters)
    for b in range(iters):
        run(b)
    torch.cuda.synchronize(dev)
    ms = pipe.frontend_times(iters)
    info = pipe.info
    pipe.close()
    return {"kernel": "k_frontend_tuned" if nsrc else "k_frontend2", "channels": nch, "rows": nsrc or nch,
            "launches": len(ms), "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4),
            "input_MB": round((nsrc or nch) * 2 * info.block_iq / 1e6, 1)}


def tuned_stepper(nsrc: int):
    class TunedStepper(bench.GpuStepper):
        def __init__(self, args, nch, first, local, nblocks):
            super().__init__(args, nch, first, local, nblocks)
            pipe = self.pipe
            pipe.set_tuning(*tuning(nch, nsrc), nsrc)
            pipe.frontend = lambda iq, stream=None: pipe.frontend_tuned(iq[:nsrc], stream=stream)
    return TunedStepper


def pipeline_step(args, factory, fill_parts: str) -> dict:
    os.environ["SDR_BENCH_FILL_PARTS"] = fill_parts
    ns = argparse.Namespace(gpus=1, steps=args.steps, warmup=args.warmup, channels=args.channels, full=False,
                            dump_outputs=None, no_cpu_baseline=True, no_gather=True, no_isolated=True,
                            backend="nccl", numerics="exact")
    res = bench.run_rank(ns, 1, 0, 0, stepper_factory=factory)
    return {"ms_per_step": res["ms_per_step"], "value_MSps": res["value"], "pll_mode": res.get("pll", {}).get("mode")}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3, help="interleaved repeats of the pipeline legs")
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r07" / "tuner"))
    args = ap.parse_args()
    import torch
    pkg = bench._load_pkg()
    dev = torch.device("cuda", 0)
    out = pathlib.Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    lines = []

    def emit(d: dict) -> None:
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    iq = bench.make_input(torch, args.channels, 8, 0, dev)
    for nsrc in (None, args.rows, args.channels, None):
        emit({"leg": "kernel_alone", **kernel_alone(torch, pkg, iq, args.channels, nsrc, args.iters)})
    del iq
    torch.cuda.empty_cache()
    if not args.skip_pipeline:
        legs = (("untuned_fill4", None, "4"), ("untuned_fill1", None, "1"),
                ("tuned_fill1", tuned_stepper(args.rows), "1"))
        got: dict = {n: [] for n, _, _ in legs}
        for rep in range(args.repeat):
            for name, factory, parts in legs:
                r = pipeline_step(args, factory, parts)
                got[name].append(r["ms_per_step"])
                emit({"leg": "pipeline_step", "name": name, "repeat": rep, "channels": args.channels,
                      "rows": args.rows if factory else args.channels, **r})
        med = {n: statistics.median(v) for n, v in got.items()}
        emit({"leg": "pipeline_ratio", "median_ms": med,
              "tuned_over_untuned_fill1": round(med["tuned_fill1"] / med["untuned_fill1"], 4),
              "tuned_over_untuned_fill4": round(med["tuned_fill1"] / med["untuned_fill4"], 4)})
    (out / "bench_tuner.jsonl").write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
