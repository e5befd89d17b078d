#!/usr/bin/env python3
"""Timing of the RDS symbol tracker (sdr_rds_track_bits, k_rds_track of sdr_rds_track.hip) in one process, mode 0.

  1. The call alone, by HIP events around `iters` back-to-back calls on one stream after a warm-up,
     interleaved over `repeat` rounds: every channel gets one block (2836 samples) per call from another of
     `ring` resident row sets (noisy chips, so the tracker is locked and decides about 36 bits a call), against
       sdr_hbm_copy             the bytes the call reads and writes (the rows, the 640-byte state in and the
                                head and carry out, nbits, the bits) through the calibration copy
  2. On the very rows a pipeline just wrote: per block a Pipeline's frontend and rds(), then sdr_rds_bits and
     sdr_rds_track_bits on that block's rds_clean, each between its own pair of events, in alternating order.
     Both read the same row (warm from the RRC, as in the engine); sdr_rds_bits cannot be called twice on a
     block, so this leg is a sum of single calls and carries each call's launch.
  3. The pipeline step on bench.py's three-stream persistent schedule (bench.run_rank with the bench's
     warm-up), interleaved: metered and decoding on the reference clock (tools/bench_rds.py's stepper), and
     the same with the tracker behind the block's RRC on the post stream and the decoder on its bits. The
     expectation under test: the ratio sits inside the run-to-run spread. There is no pass mark.

Prints one JSON line per measurement and writes them to profiles/r17/track/bench_rds_track.jsonl (--out).
  python tools/bench_rds_track.py [--channels 1024] [--iters 200] [--repeat 5] [--steps 100] [--warmup 40]
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
from bench_rds import DecodingStepper  # noqa: E402
from bench_scan import timed  # noqa: E402

WARM = 40
ROW = 2836
STATE_BYTES = 640


def noisy_rows(np, nch: int, ring: int):
    """[ring][nch][ROW] f32: consecutive blocks of 16 different chip streams with noise, repeated over the
    channels (S = 39 samples a chip, differential biphase)."""
    rs = np.random.Generator(np.random.PCG64(17))
    distinct, total = min(nch, 16), ring * ROW
    nbits = total // 78 + 2
    level = np.cumsum(rs.integers(0, 2, (distinct, nbits)), axis=1) & 1
    v = np.where(level == 1, 0.3, -0.3).astype(np.float32)
    chips = np.stack([v, -v], axis=2).reshape(distinct, 2 * nbits)
    x = np.repeat(chips, 39, axis=1)[:, :total] + rs.normal(0.0, 0.2, (distinct, total)).astype(np.float32)
    return np.ascontiguousarray(x[np.arange(nch) % distinct].reshape(nch, ring, ROW).transpose(1, 0, 2))


def calls_alone(torch, pkg, nch: int, iters: int, repeat: int, ring: int, emit) -> None:
    import numpy as np
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    rows = torch.from_numpy(noisy_rows(np, nch, ring)).to(dev)
    trk = pkg.RdsTracker(nch)
    b_in = nch * (4 * ROW + STATE_BYTES)
    b_out = nch * (88 + 240 + 4 + 37)
    n16 = (b_in + b_out + 15) // 16 * 16
    src, dst = torch.empty(ring, n16, dtype=torch.uint8, device=dev), torch.empty(n16, dtype=torch.uint8, device=dev)
    legs = {
        "sdr_rds_track_bits": lambda b: trk.feed(rows[b % ring], ROW, stream=s),
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
                  "us_per_call": round(ms * 1e3, 2), "MB": round((b_in + b_out) / 1e6, 2)})
    st = trk.stats(stream=s)
    med = {k: statistics.median(v) for k, v in got.items()}
    ratio = med["sdr_rds_track_bits"] / med["sdr_hbm_copy_bytes"]
    emit({"leg": "call_alone_summary", "channels": nch, "median_us": {k: round(v * 1e3, 2) for k, v in med.items()},
          "min_us": {k: round(min(v) * 1e3, 2) for k, v in got.items()},
          "max_us": {k: round(max(v) * 1e3, 2) for k, v in got.items()}, "MB_in": round(b_in / 1e6, 2),
          "track_over_copy": round(ratio, 2), "GBps_read": round(b_in / med["sdr_rds_track_bits"] / 1e6, 1),
          "tracker": {"locked_channels": int(st["locked"].sum()), "bits": int(st["bits"].sum()),
                      "moves": int(st["moves"].sum()), "half_moves": int(st["half_moves"].sum())}})
    trk.close()


def on_pipeline_rows(torch, pkg, nch: int, blocks: int, emit) -> None:
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    ring = 8
    iq = bench.make_input(torch, nch, ring, 0, dev)
    pipe, trk = pkg.Pipeline(nch), pkg.RdsTracker(nch)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(blocks)]
    with torch.cuda.stream(s):
        for b in range(blocks):
            pipe.frontend(iq[b % ring], stream=s)
            clean = pipe.rds(bits=False, stream=s)
            first, second = (pipe.rds_bits, lambda **k: trk.feed(clean, stream=s)) if b % 2 == 0 else \
                            (lambda **k: trk.feed(clean, stream=s), pipe.rds_bits)
            ev[b][0].record(s)
            first(stream=s)
            ev[b][1].record(s)
            second(stream=s)
            ev[b][2].record(s)
    torch.cuda.synchronize(dev)
    t = {"sdr_rds_bits": [], "sdr_rds_track_bits": []}
    for b in range(16, blocks):                    # past the reference path's six silent blocks and the warm-up
        a, c = ev[b][0].elapsed_time(ev[b][1]) * 1e3, ev[b][1].elapsed_time(ev[b][2]) * 1e3
        t["sdr_rds_bits" if b % 2 == 0 else "sdr_rds_track_bits"].append(a)
        t["sdr_rds_track_bits" if b % 2 == 0 else "sdr_rds_bits"].append(c)
    med = {k: statistics.median(v) for k, v in t.items()}
    emit({"leg": "on_pipeline_rows", "channels": nch, "blocks": blocks - 16,
          "median_us": {k: round(v, 2) for k, v in med.items()},
          "min_us": {k: round(min(v), 2) for k, v in t.items()}, "max_us": {k: round(max(v), 2) for k, v in t.items()},
          "track_over_bits": round(med["sdr_rds_track_bits"] / med["sdr_rds_bits"], 2)})
    trk.close()
    pipe.close()


class TrackingStepper(DecodingStepper):
    """The metered, decoding stepper with the tracker behind the block's RRC on the post stream, and the
    decoder on the tracker's bits."""

    def __init__(self, args, nch, first, local, nblocks):
        super().__init__(args, nch, first, local, nblocks)
        self.trk = self.pkg.RdsTracker(nch, device=local)

    def step(self, b, gather=None):
        bench.GpuStepper.step(self, b, gather)
        s = self.s_post
        s.wait_event(self.post_done[b])
        self.meter.audio(self.pipe, self.lr[b % 2], stream=s)
        self.meter.rds(self.pipe, stream=s)
        nbits, bits = self.trk.feed(self.clean, stream=s)
        self.dec.feed(nbits, bits, stream=s)
        self.post_done[b].record(s)

    def close(self):
        self.torch.cuda.synchronize(self.dev)
        self.trk.close()
        super().close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--ring", type=int, default=8, help="resident row sets the calls alone rotate over")
    ap.add_argument("--blocks", type=int, default=80, help="blocks of the leg on a pipeline's rows")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=5, help="interleaved repeats of every leg")
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r17" / "track"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rds_track: needs a GPU")
    pkg = bench._load_pkg()
    out = pathlib.Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    lines = []

    def emit(d: dict) -> None:
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        (out / "bench_rds_track.jsonl").write_text("\n".join(lines) + "\n")

    if not args.skip_calls:
        calls_alone(torch, pkg, args.channels, args.iters, args.repeat, args.ring, emit)
        torch.cuda.empty_cache()
        on_pipeline_rows(torch, pkg, args.channels, args.blocks, emit)
        torch.cuda.empty_cache()
    if not args.skip_pipeline:
        legs = (("decoding_ref_clock", DecodingStepper), ("decoding_track_clock", TrackingStepper))
        got: dict = {n: [] for n, _ in legs}
        for rep in range(min(args.repeat, 3)):
            for name, factory in legs:
                r = bench_tuner.pipeline_step(args, factory, "4")
                got[name].append(r["ms_per_step"])
                emit({"leg": "pipeline_step", "name": name, "repeat": rep, "channels": args.channels, **r})
        med = {n: statistics.median(v) for n, v in got.items()}
        spread = {n: [min(v), max(v)] for n, v in got.items()}
        ratio = med["decoding_track_clock"] / med["decoding_ref_clock"]
        # inside the spread: the two legs' ranges over the interleaved repeats overlap
        emit({"leg": "pipeline_ratio", "median_ms": med, "spread_ms": spread, "track_over_ref": round(ratio, 4),
              "added_us_per_step": round((med["decoding_track_clock"] - med["decoding_ref_clock"]) * 1e3, 2),
              "inside_spread": bool(spread["decoding_track_clock"][0] <= spread["decoding_ref_clock"][1])})


if __name__ == "__main__":
    main()
