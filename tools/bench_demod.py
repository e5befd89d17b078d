#!/usr/bin/env python3
"""Cost of the phase discriminator (SDR_FLAG_PHASE_DEMOD) against the default one, in one process.

  1. The front-end kernels alone, by their workgroup stamps (sdr_frontend_timing): k_frontend2 at 1024
     channels and k_frontend_tuned at 1024 channels on 128 source rows (tools/bench_tuner.py's shapes),
     each with and without the flag; the median of --iters launches after 40, over --repeat interleaved
     rounds. Each launch reads another resident input block.
  2. The full pipeline step on bench.py's three-stream persistent schedule (bench.run_rank, as
     tools/bench_tuner.py runs it), untuned (first block in 4 parts, as the bench) and tuned (no fill by
     parts), phase against default, --repeat interleaved repeats.

Prints one JSON line per measurement and writes them to profiles/r15/demod/ (--out).
  python tools/bench_demod.py [--channels 1024] [--rows 128] [--steps 100] [--warmup 40] [--repeat 3]
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


def kernel_alone(torch, pkg, iq, nch: int, nsrc: int | None, phase: bool, iters: int) -> dict:
    dev = iq.device
    pipe = pkg.Pipeline(nch, flags=pkg.PHASE_DEMOD if phase else 0)
    if nsrc:
        pipe.set_tuning(*bench_tuner.tuning(nch, nsrc), nsrc)
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
    pipe.close()
    return {"kernel": "k_frontend_tuned" if nsrc else "k_frontend2", "demod": "phase" if phase else "ref",
            "channels": nch, "rows": nsrc or nch, "launches": len(ms), "ms_median": round(statistics.median(ms), 4),
            "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def phase_stepper(base):
    """`base` (bench.GpuStepper or a subclass) whose context is created with SDR_FLAG_PHASE_DEMOD."""
    class PhaseStepper(base):
        def __init__(self, *a):
            pkg = bench._load_pkg()
            plain = pkg.Pipeline
            pkg.Pipeline = lambda *x, **k: plain(*x, **{**k, "flags": k.get("flags", 0) | pkg.PHASE_DEMOD})
            try:
                super().__init__(*a)
            finally:
                pkg.Pipeline = plain
    return PhaseStepper


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3, help="interleaved rounds of every leg")
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r15" / "demod"))
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

    def ratios(leg: str, got: dict, pairs) -> None:
        med = {n: statistics.median(v) for n, v in got.items()}
        emit({"leg": leg, "median_ms": {n: round(v, 4) for n, v in med.items()},
              "spread_ms": {n: round(max(v) - min(v), 4) for n, v in got.items()},
              **{f"{p}_over_{r}": round(med[p] / med[r], 4) for p, r in pairs}})

    iq = bench.make_input(torch, args.channels, 8, 0, dev)
    shapes = (("k_frontend2_ref", None, False), ("k_frontend2_phase", None, True),
              ("k_frontend_tuned_ref", args.rows, False), ("k_frontend_tuned_phase", args.rows, True))
    got: dict = {n: [] for n, _, _ in shapes}
    for rep in range(args.repeat):
        for name, nsrc, phase in shapes:
            r = kernel_alone(torch, pkg, iq, args.channels, nsrc, phase, args.iters)
            got[name].append(r["ms_median"])
            emit({"leg": "kernel_alone", "name": name, "repeat": rep, **r})
    ratios("kernel_ratio", got, (("k_frontend2_phase", "k_frontend2_ref"), ("k_frontend_tuned_phase", "k_frontend_tuned_ref")))
    del iq
    torch.cuda.empty_cache()
    if not args.skip_pipeline:
        tuned = bench_tuner.tuned_stepper(args.rows)
        legs = (("untuned_ref", None, "4"), ("untuned_phase", phase_stepper(bench.GpuStepper), "4"),
                ("tuned_ref", tuned, "1"), ("tuned_phase", phase_stepper(tuned), "1"))
        got = {n: [] for n, _, _ in legs}
        for rep in range(args.repeat):
            for name, factory, parts in legs:
                r = bench_tuner.pipeline_step(args, factory, parts)
                got[name].append(r["ms_per_step"])
                emit({"leg": "pipeline_step", "name": name, "repeat": rep, "channels": args.channels, **r})
        ratios("pipeline_ratio", got, (("untuned_phase", "untuned_ref"), ("tuned_phase", "tuned_ref")))
    (out / "bench_demod.jsonl").write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
