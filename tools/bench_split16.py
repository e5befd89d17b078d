#!/usr/bin/env python3
"""Timing of the 16-bit wideband splitter (sdr_split16_block) in one process, mode 0, on the protocol and the
shapes of tools/bench_split.py: W = 10 with 7 wide streams (133 rows) and W = 8 with 9 (135 rows).

  1. Calls alone, by HIP events around `iters` back-to-back calls on one stream after a warm-up (each call
     reads another resident wide block of random samples), interleaved over `repeat` rounds:
       sdr_split16_block        k_split16, int16 wide block -> rows
       sdr_hbm_copy             the same input bytes plus the same output bytes through the calibration copy
                                kernel (two copies back to back): the byte floor
       sdr_split_block          k_split at the same W and nwide (half the input bytes, half the MFMAs)
       sdr_frontend_tuned       1024 channels on the rows the splitter produced: the consumer
     and the 16-bit splitter as a ratio to each.
  2. The tuned pipeline step on tools/bench_tuner.py's schedule (1024 channels on as many rows), interleaved:
     with no splitter, and with a Splitter16.block per block on the front-end stream (where the receiver engine
     runs it). Reported: the ratio of the medians beside the run-to-run spread (max / min) of either leg in this
     session, and whether the ratio lies inside that spread.

Prints one JSON line per measurement and writes them to profiles/r20/split16/bench_split16.jsonl (--out).
  python tools/bench_split16.py [--channels 1024] [--iters 200] [--repeat 5] [--steps 100] [--warmup 40]
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
from bench_split import RING, SHAPES, WARM, wide_blocks  # noqa: E402


def wide16_blocks(torch, W: int, nwide: int, block_iq: int, dev):
    g = torch.Generator(device="cpu").manual_seed(1600 + W)
    x = torch.randint(-32768, 32768, (RING, nwide, 2 * W * block_iq), dtype=torch.int16, generator=g)
    return x.to(dev)


def calls_alone(torch, pkg, W: int, nwide: int, nch: int, iters: int, repeat: int, emit) -> None:
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    sp, sp8 = pkg.Splitter16(W, nwide), pkg.Splitter(W, nwide)
    nsrc = nwide * sp.rows
    wide, wide8 = wide16_blocks(torch, W, nwide, sp.block_iq, dev), wide_blocks(torch, W, nwide, sp.block_iq, dev)
    rows = [torch.empty(nsrc, 2 * sp.block_iq, dtype=torch.uint8, device=dev) for _ in range(2)]
    for b in range(2):
        sp.block(wide[b], out=rows[b], stream=s)
    pipe = pkg.Pipeline(nch)
    pipe.set_tuning(*bench_tuner.tuning(nch, nsrc), nsrc)
    in_bytes, out_bytes = wide[0].numel() * 2, rows[0].numel()
    c_in = torch.empty(RING, (in_bytes + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    c_out = torch.empty(RING, (out_bytes + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    d_in, d_out = torch.empty_like(c_in[0]), torch.empty_like(c_out[0])

    def copies(b):
        pkg.hbm_copy(d_in, c_in[b % RING], stream=s)
        pkg.hbm_copy(d_out, c_out[b % RING], stream=s)

    legs = {
        "sdr_split16_block": lambda b: sp.block(wide[b % RING], out=rows[b & 1], stream=s),
        "sdr_hbm_copy": copies,
        "sdr_split_block": lambda b: sp8.block(wide8[b % RING], out=rows[b & 1], stream=s),
        "sdr_frontend_tuned": lambda b: pipe.frontend_tuned(rows[b & 1], stream=s),
    }
    got: dict = {k: [] for k in legs}
    for name, call in legs.items():
        for b in range(WARM):
            call(b)
    torch.cuda.synchronize(dev)
    for rep in range(repeat):
        for name, call in legs.items():
            ms = timed(torch, s, call, iters)
            got[name].append(ms)
            emit({"leg": "call_alone", "call": name, "W": W, "nwide": nwide, "rows": nsrc, "repeat": rep, "iters": iters,
                  "channels": nch if name == "sdr_frontend_tuned" else None, "ms_per_call": round(ms, 4)})
    med = {k: statistics.median(v) for k, v in got.items()}
    T, R = 16 * W, 2 * W - 1
    macs = nwide * sp.block_iq * 2 * T * 2 * R                  # useful int16 x int16 multiply-adds
    cols = (2 * R + 15) // 16 * 16
    m16 = med["sdr_split16_block"]
    emit({"leg": "call_alone_summary", "W": W, "nwide": nwide, "rows": nsrc,
          "median_ms": {k: round(v, 4) for k, v in med.items()},
          "min_ms": {k: round(min(v), 4) for k, v in got.items()},
          "max_ms": {k: round(max(v), 4) for k, v in got.items()},
          "input_MB": round(in_bytes / 1e6, 2), "output_MB": round(out_bytes / 1e6, 2),
          "split16_GBps_in_plus_out": round((in_bytes + out_bytes) / m16 / 1e6, 1),
          "copy_GBps_in_plus_out": round((in_bytes + out_bytes) / med["sdr_hbm_copy"] / 1e6, 1),
          "split16_over_copy": round(m16 / med["sdr_hbm_copy"], 2),
          "split16_over_split8": round(m16 / med["sdr_split_block"], 2),
          "split16_over_frontend_tuned": round(m16 / med["sdr_frontend_tuned"], 3),
          "useful_GMAC": round(macs / 1e9, 2),
          "mfma_i8_GMAC": round(macs / (2 * R) * cols * 4 / 1e9, 2),     # four planes, padded columns
          "useful_TMACps": round(macs / m16 / 1e9, 2),
          "clips": int(sp.clips(stream=s).sum()), "peak_max": int(sp.peaks(stream=s).max())})
    sp.close()
    sp8.close()
    pipe.close()


def split16_stepper(W: int, nwide: int):
    """bench_tuner's tuned stepper plus a Splitter16.block per block on the front-end stream."""
    nsrc = nwide * (2 * W - 1)
    base = bench_tuner.tuned_stepper(nsrc)

    class Split16Stepper(base):
        def __init__(self, args, nch, first, local, nblocks):
            super().__init__(args, nch, first, local, nblocks)
            self.split = self.pkg.Splitter16(W, nwide, device=local)
            self.wide = wide16_blocks(self.torch, W, nwide, self.split.block_iq, self.dev)
            self.split_rows = self.torch.empty(nsrc, 2 * self.split.block_iq, dtype=self.torch.uint8, device=self.dev)

        def step(self, b, gather=None):
            super().step(b, gather)
            self.split.block(self.wide[b % RING], out=self.split_rows, stream=self.s_fe)

        def close(self):
            self.torch.cuda.synchronize(self.dev)
            self.split.close()
            super().close()
    return Split16Stepper


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=5, help="interleaved repeats of every leg")
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r20" / "split16"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_split16: needs a GPU")
    pkg = bench._load_pkg()
    out = pathlib.Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    lines = []

    def emit(d: dict) -> None:
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        (out / "bench_split16.jsonl").write_text("\n".join(lines) + "\n")

    for W, nwide in SHAPES:
        calls_alone(torch, pkg, W, nwide, args.channels, args.iters, args.repeat, emit)
        torch.cuda.empty_cache()
    if not args.skip_pipeline:
        for W, nwide in SHAPES:
            nsrc = nwide * (2 * W - 1)
            legs = (("tuned_no_split", bench_tuner.tuned_stepper(nsrc)), ("tuned_split16_on_fe_stream", split16_stepper(W, nwide)))
            got: dict = {n: [] for n, _ in legs}
            for rep in range(min(args.repeat, 3)):
                for name, factory in legs:
                    r = bench_tuner.pipeline_step(args, factory, "1")
                    got[name].append(r["ms_per_step"])
                    emit({"leg": "pipeline_step", "name": name, "W": W, "nwide": nwide, "repeat": rep,
                          "channels": args.channels, "rows": nsrc, **r})
            med = {n: statistics.median(v) for n, v in got.items()}
            spread = {n: round(max(v) / min(v), 4) for n, v in got.items()}
            ratio = med["tuned_split16_on_fe_stream"] / med["tuned_no_split"]
            emit({"leg": "pipeline_ratio", "W": W, "nwide": nwide, "median_ms": med,
                  "split16_on_fe_over_none": round(ratio, 4), "run_to_run_spread_max_over_min": spread,
                  "ratio_inside_spread": bool(max(ratio, 1.0 / ratio) <= max(spread.values()))})


if __name__ == "__main__":
    main()
