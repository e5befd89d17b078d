#!/usr/bin/env python3
"""Timing of the RF meter (SDR_FLAG_IF_ENVELOPE, sdr_meter_rf) in one process, 1024 channels, mode 0.

  1. The front-end kernels alone, by their own workgroup stamps (sdr_frontend_timing), with and without the
     flag, interleaved over `repeat` rounds: k_frontend2 at 1024 channels, and k_frontend_tuned at 1024 channels
     on 128 source rows. Each launch reads another resident input block. With the flag a launch also writes
     the if_env rows (4 * block_if bytes per channel: 30.1 MB at 1024 channels).
  2. sdr_meter_rf alone, by HIP events around `iters` back-to-back calls on one stream after a warm-up, each
     call on another of `ring` resident contexts, against sdr_hbm_copy of the bytes it reads (the byte floor:
     the copy also writes them, the meter writes 32 bytes a channel).
  3. The metered pipeline step on bench.py's three-stream persistent schedule (tools/bench_meter.py's
     MeteredStepper), interleaved: as it is, and with the flag on the context and sdr_meter_rf per block on the
     post stream beside the other two meter calls.

Prints one JSON line per measurement and writes them to profiles/r21/rf/bench_rf.jsonl (--out).
  python tools/bench_rf.py [--channels 1024] [--rows 128] [--iters 50] [--repeat 5] [--steps 100] [--warmup 40]
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
from bench_meter import MeteredStepper  # noqa: E402
from bench_scan import timed  # noqa: E402

WARM = 40


def kernel_alone(torch, pkg, iq, nch: int, nsrc: int | None, flags: int, iters: int) -> list:
    """ms of `iters` stamped launches of the untuned (nsrc None) or tuned front end of a context with `flags`."""
    dev = iq.device
    pipe = pkg.Pipeline(nch, flags=flags)
    if nsrc:
        pipe.set_tuning(*bench_tuner.tuning(nch, nsrc), nsrc)
    s = torch.cuda.Stream(dev)
    run = (lambda b: pipe.frontend_tuned(iq[b % iq.shape[0], :nsrc], stream=s)) if nsrc else \
          (lambda b: pipe.frontend(iq[b % iq.shape[0]], stream=s))
    for b in range(WARM):
        run(b)
    torch.cuda.synchronize(dev)
    pipe.frontend_timing(iters)
    for b in range(iters):
        run(b)
    torch.cuda.synchronize(dev)
    ms = pipe.frontend_times(iters)
    pipe.close()
    return ms


def kernels(torch, pkg, iq, nch: int, rows: int, iters: int, repeat: int, emit) -> None:
    legs = [("k_frontend2", None, 0), ("k_frontend2+env", None, pkg.IF_ENVELOPE),
            ("k_frontend_tuned", rows, 0), ("k_frontend_tuned+env", rows, pkg.IF_ENVELOPE)]
    got: dict = {n: [] for n, _, _ in legs}
    for rep in range(repeat):
        for name, nsrc, flags in legs:
            ms = kernel_alone(torch, pkg, iq, nch, nsrc, flags, iters)
            got[name].append(statistics.median(ms))
            emit({"leg": "kernel_alone", "kernel": name, "repeat": rep, "channels": nch, "rows": nsrc or nch,
                  "launches": len(ms), "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                  "ms_max": round(max(ms), 4)})
    med = {k: statistics.median(v) for k, v in got.items()}
    emit({"leg": "kernel_alone_summary", "channels": nch, "median_ms": {k: round(v, 4) for k, v in med.items()},
          "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in got.items()},
          "untuned_env_over_plain": round(med["k_frontend2+env"] / med["k_frontend2"], 4),
          "tuned_env_over_plain": round(med["k_frontend_tuned+env"] / med["k_frontend_tuned"], 4)})


def call_alone(torch, pkg, iq, nch: int, iters: int, repeat: int, ring: int, emit) -> None:
    dev = iq.device
    s = torch.cuda.Stream(dev)
    pipes = []
    for r in range(ring):                      # one block through every context: its row is the call's input
        pipe = pkg.Pipeline(nch, flags=pkg.IF_ENVELOPE)
        pipe.frontend(iq[r % iq.shape[0]], stream=s)
        pipes.append(pipe)
    meter = pkg.Meter(nch)
    nbytes = nch * 4 * pipes[0].info.block_if
    n16 = (nbytes + 15) // 16 * 16
    src, dst = torch.empty(ring, n16, dtype=torch.uint8, device=dev), torch.empty(n16, dtype=torch.uint8, device=dev)
    legs = {"sdr_meter_rf": lambda b: meter.rf(pipes[b % ring], stream=s),
            "sdr_hbm_copy_rf_bytes": lambda b: pkg.hbm_copy(dst, src[b % ring], stream=s)}
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
                  "ms_per_call": round(ms, 4), "read_MB": round(nbytes / 1e6, 1), "GBps_read": round(nbytes / ms / 1e6, 1)})
    med = {k: statistics.median(v) for k, v in got.items()}
    emit({"leg": "call_alone_summary", "channels": nch, "median_ms": {k: round(v, 4) for k, v in med.items()},
          "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in got.items()},
          "rf_over_copy": round(med["sdr_meter_rf"] / med["sdr_hbm_copy_rf_bytes"], 2)})
    torch.cuda.synchronize(dev)
    meter.close()
    for pipe in pipes:
        pipe.close()


class RfMeteredStepper(MeteredStepper):
    """The metered stepper on a context with the flag, plus sdr_meter_rf of every block beside the other two meter
    calls on the post stream (the block's if_env row lives until the front end of the block two later, which waits
    for this reader)."""

    def __init__(self, args, nch, first, local, nblocks):
        pkg = bench._load_pkg()
        plain = pkg.Pipeline
        pkg.Pipeline = lambda *a, **k: plain(*a, **{**k, "flags": k.get("flags", 0) | pkg.IF_ENVELOPE})
        try:
            super().__init__(args, nch, first, local, nblocks)
        finally:
            pkg.Pipeline = plain

    def step(self, b, gather=None):
        super().step(b, gather)
        self.meter.rf(self.pipe, stream=self.s_post)
        self.post_done[b].record(self.s_post)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ring", type=int, default=4, help="resident contexts sdr_meter_rf alone rotates over")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=5, help="interleaved repeats of every leg")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r21" / "rf"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rf: needs a GPU")
    pkg = bench._load_pkg()
    dev = torch.device("cuda", 0)
    out = pathlib.Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    lines = []

    def emit(d: dict) -> None:
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        (out / "bench_rf.jsonl").write_text("\n".join(lines) + "\n")

    if not (args.skip_kernels and args.skip_calls):
        iq = bench.make_input(torch, args.channels, 8, 0, dev)
        if not args.skip_kernels:
            kernels(torch, pkg, iq, args.channels, args.rows, args.iters, args.repeat, emit)
        if not args.skip_calls:
            call_alone(torch, pkg, iq, args.channels, 4 * args.iters, args.repeat, args.ring, emit)
        del iq
        torch.cuda.empty_cache()
    if not args.skip_pipeline:
        legs = (("metered", MeteredStepper), ("metered_rf", RfMeteredStepper))
        got: dict = {n: [] for n, _ in legs}
        for rep in range(min(args.repeat, 3)):
            for name, factory in legs:
                r = bench_tuner.pipeline_step(args, factory, "4")
                got[name].append(r["ms_per_step"])
                emit({"leg": "pipeline_step", "name": name, "repeat": rep, "channels": args.channels, **r})
        med = {n: statistics.median(v) for n, v in got.items()}
        emit({"leg": "pipeline_ratio", "median_ms": med, "spread_ms": {n: [min(v), max(v)] for n, v in got.items()},
              "rf_over_metered": round(med["metered_rf"] / med["metered"], 4)})


if __name__ == "__main__":
    main()
