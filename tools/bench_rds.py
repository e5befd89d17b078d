#!/usr/bin/env python3
"""Timing of the RDS group decoder (sdr_rds_groups, k_rds_groups of sdr_rds.hip) in one process, mode 0.

  1. The call alone, by HIP events around `iters` back-to-back calls on one stream after a warm-up,
     interleaved over `repeat` rounds: every channel gets one block's bits per call, 36 and 37 alternating
     (a clean 0A stream per channel, so the decoder is synchronised and walks judgement points), against
       sdr_hbm_copy             the bytes the call reads and writes (nbits, the bit rows' used part, the
                                128-byte state in and out, the group records) through the calibration copy
     Both move a few hundred kilobytes per call at 1024 channels, far too few for bytes to matter: the copy's
     time is a launch's. The summary names what bounds the decoder: "launch" when it takes less than twice
     the copy's time, else "one wave's dependent chain" (a channel is one wave that loads its state, its
     bits and, on a failing block, a table entry one after the other, and then walks alone).
  2. The pipeline step on bench.py's three-stream persistent schedule (bench.run_rank with the bench's
     warm-up), interleaved: metered (tools/bench_meter.py's stepper), and metered with the decoder behind
     the block's bits on the post stream. The expectation under test: the ratio sits inside the run-to-run
     spread (the two legs' ranges overlap). There is no pass mark; the figures are reported.

Prints one JSON line per measurement and writes them to profiles/r16/rds/bench_rds.jsonl (--out).
  python tools/bench_rds.py [--channels 1024] [--iters 400] [--repeat 5] [--steps 100] [--warmup 40]
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
CALLS = 64            # resident calls the timed loop rotates over (36, 37, 36, ...: 2336 bits per channel)


def call_rows(np, synth, nch: int):
    """nbits [CALLS][nch] and bits [CALLS][nch][256] of clean 0A streams, one per channel."""
    sizes = [36 + (k & 1) for k in range(CALLS)]
    total = sum(sizes)
    distinct = min(nch, 16)                       # 16 different stations, repeated over the channels
    # rds_bitstream is differentially ENcoded: the decoder's input is the decoded stream, b[n] = d[n] ^ d[n-1]
    enc = np.stack([synth.rds_bitstream_fast(c, total) for c in range(distinct)])
    dec = enc.copy()
    dec[:, 1:] ^= enc[:, :-1]
    streams = dec.astype(np.uint8)
    rows = np.zeros((CALLS, nch, 256), np.uint8)
    at = 0
    for k, n in enumerate(sizes):
        rows[k, :, :n] = streams[np.arange(nch) % distinct, at:at + n]
        at += n
    nbits = np.repeat(np.array(sizes, np.int32)[:, None], nch, axis=1)
    return nbits, rows


def calls_alone(torch, pkg, nch: int, iters: int, repeat: int, emit) -> None:
    import numpy as np
    import real_time_sdr_amd.synth as synth
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    nbits, rows = call_rows(np, synth, nch)
    d_nbits, d_rows = torch.from_numpy(nbits).to(dev), torch.from_numpy(rows).to(dev)
    dec = pkg.RdsDecoder(nch)
    # per call and channel: nbits 4, bits 37, state 128 in + 128 out, ngroups 4, a group now and then 16
    nbytes = nch * (4 + 37 + 128 + 128 + 4 + 16)
    n16 = (nbytes + 15) // 16 * 16
    src, dst = torch.empty(n16, dtype=torch.uint8, device=dev), torch.empty(n16, dtype=torch.uint8, device=dev)
    legs = {
        "sdr_rds_groups": lambda b: dec.feed(d_nbits[b % CALLS], d_rows[b % CALLS], stream=s),
        "sdr_hbm_copy_bytes": lambda b: pkg.hbm_copy(dst, src, stream=s),
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
            emit({"leg": "call_alone", "call": name, "repeat": rep, "channels": nch, "iters": iters,
                  "us_per_call": round(ms * 1e3, 2), "KB": round(nbytes / 1e3, 1)})
    st = dec.stats(stream=s)
    med = {k: statistics.median(v) for k, v in got.items()}
    ratio = med["sdr_rds_groups"] / med["sdr_hbm_copy_bytes"]
    emit({"leg": "call_alone_summary", "channels": nch, "median_us": {k: round(v * 1e3, 2) for k, v in med.items()},
          "min_us": {k: round(min(v) * 1e3, 2) for k, v in got.items()},
          "max_us": {k: round(max(v) * 1e3, 2) for k, v in got.items()}, "KB": round(nbytes / 1e3, 1),
          "groups_over_copy": round(ratio, 2),
          "GBps_of_those_bytes": round(nbytes / med["sdr_rds_groups"] / 1e6, 2),
          "bound": "launch" if ratio < 2.0 else "one wave's dependent chain",
          "decoder": {"synced_channels": int(st["synced"].sum()), "groups": int(st["groups"].sum()),
                      "bad": int(st["bad"].sum()), "lost": int(st["lost"].sum())}})
    dec.close()


class DecodingStepper(MeteredStepper):
    """The metered stepper plus the group decoder on the post stream, behind the block's bits."""

    def __init__(self, args, nch, first, local, nblocks):
        super().__init__(args, nch, first, local, nblocks)
        self.dec = self.pkg.RdsDecoder(nch, device=local)

    def step(self, b, gather=None):
        super().step(b, gather)
        s = self.s_post
        s.wait_event(self.post_done[b])
        self.dec.feed(self.pipe.nbits, self.bits[b % 2], stream=s)
        self.post_done[b].record(s)

    def close(self):
        self.torch.cuda.synchronize(self.dev)
        self.dec.close()
        super().close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=5, help="interleaved repeats of every leg")
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r16" / "rds"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rds: needs a GPU")
    pkg = bench._load_pkg()
    out = pathlib.Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    lines = []

    def emit(d: dict) -> None:
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        (out / "bench_rds.jsonl").write_text("\n".join(lines) + "\n")

    if not args.skip_calls:
        calls_alone(torch, pkg, args.channels, args.iters, args.repeat, emit)
        torch.cuda.empty_cache()
    if not args.skip_pipeline:
        legs = (("metered", MeteredStepper), ("metered_decoding", DecodingStepper))
        got: dict = {n: [] for n, _ in legs}
        for rep in range(min(args.repeat, 3)):
            for name, factory in legs:
                r = bench_tuner.pipeline_step(args, factory, "4")
                got[name].append(r["ms_per_step"])
                emit({"leg": "pipeline_step", "name": name, "repeat": rep, "channels": args.channels, **r})
        med = {n: statistics.median(v) for n, v in got.items()}
        spread = {n: [min(v), max(v)] for n, v in got.items()}
        ratio = med["metered_decoding"] / med["metered"]
        # inside the spread: the two legs' ranges over the interleaved repeats overlap
        emit({"leg": "pipeline_ratio", "median_ms": med, "spread_ms": spread,
              "decoding_over_metered": round(ratio, 4),
              "added_us_per_step": round((med["metered_decoding"] - med["metered"]) * 1e3, 2),
              "inside_spread": bool(spread["metered_decoding"][0] <= spread["metered"][1])})

if __name__ == "__main__":
    main()
