#!/usr/bin/env python3
"""Timing of coherent RDS (the quadrature branch of SDR_FLAG_RDS_QUAD and sdr_rds_carrier_rotate, k_rds_carrier of
sdr_rds_carrier.hip) in one process, mode 0.

  1. The rotate call alone, by HIP events around `iters` back-to-back calls on one stream after a warm-up,
     interleaved over `repeat` rounds: every channel gets one block (2836 samples) of both rows per call from
     another of `ring` resident row sets (turned noisy chips), against
       sdr_hbm_copy             the bytes the call moves (two rows in, one out) through the calibration copy
  2. sdr_rds_post with and without the flag: two pipelines on the same input, block by block in alternating
     order, each post stage between its own pair of events (a sum of single calls: it carries their launches).
  3. The pipeline step on bench.py's three-stream persistent schedule (bench.run_rank with the bench's
     warm-up), interleaved: metered and decoding on the tracker's clock (tools/bench_rds_track.py's stepper, the
     path without the option), and the same with the quadrature branch, the derotator in front of the tracker.
     The ratio is reported beside the run-to-run spread. There is no pass mark.

Prints one JSON line per measurement and writes them to profiles/r19/carrier/bench_rds_carrier.jsonl (--out).
  python tools/bench_rds_carrier.py [--channels 1024] [--iters 200] [--repeat 5] [--steps 100] [--warmup 40]
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
from bench_rds_track import TrackingStepper, noisy_rows  # noqa: E402
from bench_scan import timed  # noqa: E402

WARM = 40
ROW = 2836


def calls_alone(torch, pkg, nch: int, iters: int, repeat: int, ring: int, emit) -> None:
    import numpy as np
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    x = noisy_rows(np, nch, ring)
    c, sn = np.float32(np.cos(np.deg2rad(-44.5))), np.float32(np.sin(np.deg2rad(-44.5)))
    rows_i, rows_q = torch.from_numpy(x * c).to(dev), torch.from_numpy(x * sn).to(dev)
    out = torch.zeros(nch, ROW, dtype=torch.float32, device=dev)
    car = pkg.RdsCarrier(nch)
    nbytes = 3 * nch * ROW * 4
    n16 = (nbytes // 2 + 15) // 16 * 16               # the copy reads n16 and writes n16: the call's bytes in all
    src, dst = torch.empty(ring, n16, dtype=torch.uint8, device=dev), torch.empty(n16, dtype=torch.uint8, device=dev)
    legs = {
        "sdr_rds_carrier_rotate": lambda b: car.feed(rows_i[b % ring], rows_q[b % ring], ROW, stream=s, out=out),
        "sdr_hbm_copy_bytes": lambda b: pkg.hbm_copy(dst, src[b % ring], stream=s),
    }
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
                  "us_per_call": round(ms * 1e3, 2), "MB": round(nbytes / 1e6, 2)})
    st = car.stats(stream=s)
    med = {k: statistics.median(v) for k, v in got.items()}
    emit({"leg": "call_alone_summary", "channels": nch, "median_us": {k: round(v * 1e3, 2) for k, v in med.items()},
          "min_us": {k: round(min(v) * 1e3, 2) for k, v in got.items()},
          "max_us": {k: round(max(v) * 1e3, 2) for k, v in got.items()}, "MB": round(nbytes / 1e6, 2),
          "rotate_over_copy": round(med["sdr_rds_carrier_rotate"] / med["sdr_hbm_copy_bytes"], 2),
          "GBps": round(nbytes / med["sdr_rds_carrier_rotate"] / 1e6, 1),
          "carrier": {"phase_deg_median": round(float(np.median(pkg.rds_carrier_phase_deg(st))), 2),
                      "coherence_median": round(float(np.median(pkg.rds_carrier_coherence(st))), 3),
                      "windows": int(st["windows"].sum()), "resets": int(st["resets"].sum())}})
    car.close()


def post_with_and_without(torch, pkg, nch: int, blocks: int, emit) -> None:
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    ring = 8
    iq = bench.make_input(torch, nch, ring, 0, dev)
    pipes = {"sdr_rds_post": pkg.Pipeline(nch), "sdr_rds_post_quad": pkg.Pipeline(nch, flags=pkg.RDS_QUAD)}
    clean = torch.empty(nch, pipes["sdr_rds_post"].info.n_rds, dtype=torch.float32, device=dev)
    ev = {k: [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(blocks)] for k in pipes}
    with torch.cuda.stream(s):
        for b in range(blocks):
            order = list(pipes) if b % 2 == 0 else list(pipes)[::-1]
            for k in order:
                pipe = pipes[k]
                pipe.frontend(iq[b % ring], stream=s)
                pipe.rds_pre(stream=s)
                pipe.rds_pll(stream=s)
                ev[k][b][0].record(s)
                pipe.rds_post(clean, bits=False, stream=s)
                ev[k][b][1].record(s)
    torch.cuda.synchronize(dev)
    t = {k: [ev[k][b][0].elapsed_time(ev[k][b][1]) * 1e3 for b in range(16, blocks)] for k in pipes}
    med = {k: statistics.median(v) for k, v in t.items()}
    emit({"leg": "rds_post", "channels": nch, "blocks": blocks - 16, "median_us": {k: round(v, 2) for k, v in med.items()},
          "min_us": {k: round(min(v), 2) for k, v in t.items()}, "max_us": {k: round(max(v), 2) for k, v in t.items()},
          "quad_over_plain": round(med["sdr_rds_post_quad"] / med["sdr_rds_post"], 2),
          "added_us": round(med["sdr_rds_post_quad"] - med["sdr_rds_post"], 2)})
    for p in pipes.values():
        p.close()


class CarrierStepper(TrackingStepper):
    """The tracking stepper on a RDS_QUAD pipeline, with the derotator between the block's RRCs and the tracker."""

    def __init__(self, args, nch, first, local, nblocks):
        pkg = bench._load_pkg()
        plain = pkg.Pipeline
        # bench.GpuStepper makes its own Pipeline: give that one the flag
        pkg.Pipeline = lambda *a, **k: plain(*a, **{**k, "flags": k.get("flags", 0) | pkg.RDS_QUAD})
        try:
            super().__init__(args, nch, first, local, nblocks)
        finally:
            pkg.Pipeline = plain
        self.car = self.pkg.RdsCarrier(nch, device=local)
        self.rot = self.torch.zeros(nch, ROW, dtype=self.torch.float32, device=self.dev)

    def step(self, b, gather=None):
        bench.GpuStepper.step(self, b, gather)
        s = self.s_post
        s.wait_event(self.post_done[b])
        self.meter.audio(self.pipe, self.lr[b % 2], stream=s)
        self.meter.rds(self.pipe, stream=s)
        rows = self.car.feed_pipeline(self.pipe, self.clean, stream=s, out=self.rot)
        nbits, bits = self.trk.feed(rows, ROW, stream=s)
        self.dec.feed(nbits, bits, stream=s)
        self.post_done[b].record(s)

    def close(self):
        self.torch.cuda.synchronize(self.dev)
        self.car.close()
        super().close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--ring", type=int, default=8, help="resident row sets the calls alone rotate over")
    ap.add_argument("--blocks", type=int, default=80, help="blocks of the sdr_rds_post leg")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=5, help="interleaved repeats of every leg")
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r19" / "carrier"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rds_carrier: needs a GPU")
    pkg = bench._load_pkg()
    out = pathlib.Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    lines = []

    def emit(d: dict) -> None:
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        (out / "bench_rds_carrier.jsonl").write_text("\n".join(lines) + "\n")

    if not args.skip_calls:
        calls_alone(torch, pkg, args.channels, args.iters, args.repeat, args.ring, emit)
        torch.cuda.empty_cache()
        post_with_and_without(torch, pkg, args.channels, args.blocks, emit)
        torch.cuda.empty_cache()
    if not args.skip_pipeline:
        legs = (("decoding_track_clock", TrackingStepper), ("decoding_carrier_quad", CarrierStepper))
        got: dict = {n: [] for n, _ in legs}
        for rep in range(min(args.repeat, 3)):
            for name, factory in legs:
                r = bench_tuner.pipeline_step(args, factory, "4")
                got[name].append(r["ms_per_step"])
                emit({"leg": "pipeline_step", "name": name, "repeat": rep, "channels": args.channels, **r})
        med = {n: statistics.median(v) for n, v in got.items()}
        spread = {n: [min(v), max(v)] for n, v in got.items()}
        ratio = med["decoding_carrier_quad"] / med["decoding_track_clock"]
        # inside the spread: the two legs' ranges over the interleaved repeats overlap
        emit({"leg": "pipeline_ratio", "median_ms": med, "spread_ms": spread, "quad_over_track": round(ratio, 4),
              "added_us_per_step": round((med["decoding_carrier_quad"] - med["decoding_track_clock"]) * 1e3, 2),
              "inside_spread": bool(spread["decoding_carrier_quad"][0] <= spread["decoding_track_clock"][1])})


if __name__ == "__main__":
    main()
