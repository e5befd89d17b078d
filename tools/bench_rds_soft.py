#!/usr/bin/env python3
"""Timing of the RDS soft decisions (sdr_rds_track_bits_soft and sdr_rds_groups_soft; k_rds_track<true> and
k_rds_groups<true> of sdr_rds_track.hip and sdr_rds.hip) against the calls they extend, in one process, mode 0.

  1. The tracker's call alone: sdr_rds_track_bits and sdr_rds_track_bits_soft on two handles and the same
     resident rows, by HIP events around `iters` back-to-back calls on one stream after a warm-up, interleaved
     over `repeat` rounds. The rows are a seamless cycle of 52 calls of 36 bits (18 groups of type 0A, twice 936
     bits, so the differential level closes) as chips at amplitude 300 / 1024, once clean and once under uniform
     noise of +-2500 / 1024.
  2. The decoder's call alone: sdr_rds_groups and sdr_rds_groups_soft (soft_bits 6) on two handles and the bits
     (and soft values) the tracker made of those rows, the same way: on the clean bits, where the soft step never
     runs, and on the noisy ones, where about half the blocks take it. The counters say how many did.
  3. The pipeline step on bench.py's three-stream persistent schedule (bench.run_rank with the bench's warm-up),
     interleaved: metered, decoding and tracking (tools/bench_rds_track.py's stepper), and the same with the soft
     tracker call and the soft decoder. The claim under test: the step stays inside the run-to-run spread.
     There is no pass mark; the summary line states it as confirmed or refuted.

Prints one JSON line per measurement and writes them to profiles/r18/soft/bench_rds_soft.jsonl (--out).
  python tools/bench_rds_soft.py [--channels 1024] [--iters 200] [--repeat 5] [--steps 100] [--warmup 40]
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
from bench_rds_track import TrackingStepper  # noqa: E402
from bench_scan import timed  # noqa: E402

S, B = 39, 78
CALL_BITS, RING = 36, 52                    # 52 calls of 36 bits = 1872 bits = twice 9 groups
N = CALL_BITS * B
DISTINCT = 16


def cycle_rows(np, synth, noise_q: int):
    """[RING][DISTINCT][N] f32: the chips of twice nine 0A groups at amplitude 300 / 1024, with DISTINCT
    realisations of uniform integer noise +-noise_q / 1024."""
    blocks = []
    for k in range(9):
        blocks += synth.rds_group_0a(0x2001, 10, k & 3, "SOFT  18", af=((225 + (k & 1)) << 8) | (10 + k % 7))
    bits = [(blk >> (25 - i)) & 1 for blk in blocks for i in range(26)] * 2
    assert len(bits) == RING * CALL_BITS and sum(bits) % 2 == 0
    level = np.cumsum(bits) & 1
    v = np.where(level == 1, 300.0, -300.0).astype(np.float32)
    x = np.repeat(np.stack([v, -v], axis=1).reshape(-1), S)[None, :].repeat(DISTINCT, axis=0)
    rs = np.random.Generator(np.random.PCG64(18))
    if noise_q:
        x = x + rs.integers(-noise_q, noise_q + 1, x.shape).astype(np.float32)
    x = (x / np.float32(1024.0)).astype(np.float32)
    return np.ascontiguousarray(x.reshape(DISTINCT, RING, N).transpose(1, 0, 2))


def run_legs(torch, s, legs, iters, repeat, emit, **tags):
    got: dict = {k: [] for k in legs}
    for rep in range(repeat):
        for name, call in legs.items():
            ms = timed(torch, s, call, iters)
            got[name].append(ms)
            emit({"leg": "call_alone", "call": name, "repeat": rep, "iters": iters, "us_per_call": round(ms * 1e3, 2), **tags})
    return got


def summary(got: dict, base: str, soft: str) -> dict:
    med = {k: statistics.median(v) for k, v in got.items()}
    return {"median_us": {k: round(v * 1e3, 2) for k, v in med.items()},
            "min_us": {k: round(min(v) * 1e3, 2) for k, v in got.items()},
            "max_us": {k: round(max(v) * 1e3, 2) for k, v in got.items()},
            "soft_over_hard": round(med[soft] / med[base], 4),
            "inside_spread": bool(min(got[soft]) <= max(got[base]))}


def calls_alone(torch, pkg, np, nch: int, iters: int, repeat: int, emit) -> None:
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    chan = torch.arange(nch, device=dev) % DISTINCT
    for stream_name, noise_q in (("clean", 0), ("noise_2500", 2500)):
        rows = torch.from_numpy(cycle_rows(np, pkg.synth, noise_q)).to(dev)[:, chan].contiguous()      # [RING][nch][N]
        hard, soft = pkg.RdsTracker(nch), pkg.RdsTracker(nch)
        d_soft = torch.zeros(nch, 256, dtype=torch.int16, device=dev)
        legs = {"sdr_rds_track_bits": lambda b: hard.feed(rows[b % RING], N, stream=s),
                "sdr_rds_track_bits_soft": lambda b: soft.feed(rows[b % RING], N, stream=s, soft=d_soft)}
        for call in legs.values():
            for b in range(2 * RING):
                call(b)
        torch.cuda.synchronize(dev)
        got = run_legs(torch, s, legs, iters, repeat, emit, stream=stream_name, channels=nch)
        st = soft.stats(stream=s)
        emit({"leg": "tracker_summary", "stream": stream_name, "channels": nch, **summary(got, *legs),
              "tracker": {"locked_channels": int(st["locked"].sum()), "moves": int(st["moves"].sum())}})
        # the cycle's bits and soft values, for the decoder: the tracker is in step with the cycle only up to
        # its own delay, which is the same every round, so the recorded calls repeat seamlessly too
        soft.reset(stream=s)
        nb_all = torch.zeros(RING, nch, dtype=torch.int32, device=dev)
        bits_all = torch.zeros(RING, nch, 256, dtype=torch.uint8, device=dev)
        soft_all = torch.zeros(RING, nch, 256, dtype=torch.int16, device=dev)
        for b in range(3 * RING):
            k = b % RING
            soft.feed(rows[k], N, stream=s, nbits=nb_all[k], bits=bits_all[k], soft=soft_all[k])
        torch.cuda.synchronize(dev)
        hard.close()
        soft.close()
        del rows
        dh, ds = pkg.RdsDecoder(nch), pkg.RdsDecoder(nch, soft_bits=6)
        legs = {"sdr_rds_groups": lambda b: dh.feed(nb_all[b % RING], bits_all[b % RING], stream=s),
                "sdr_rds_groups_soft": lambda b: ds.feed(nb_all[b % RING], bits_all[b % RING], stream=s, soft=soft_all[b % RING])}
        for call in legs.values():
            for b in range(2 * RING):
                call(b)
        torch.cuda.synchronize(dev)
        before = (dh.stats(stream=s), ds.stats(stream=s), ds.soft_stats(stream=s))
        got = run_legs(torch, s, legs, iters, repeat, emit, stream=stream_name, channels=nch)
        after = (dh.stats(stream=s), ds.stats(stream=s), ds.soft_stats(stream=s))

        def delta(i, name):
            return int(after[i][name].astype(np.int64).sum() - before[i][name].astype(np.int64).sum())

        blocks_soft = sum(delta(1, n) for n in ("good", "corrected", "bad"))
        emit({"leg": "decoder_summary", "stream": stream_name, "channels": nch, **summary(got, *legs),
              "hard": {n: delta(0, n) for n in ("good", "corrected", "bad", "lost", "groups")},
              "soft": {n: delta(1, n) for n in ("good", "corrected", "bad", "lost", "groups")},
              "soft_blocks": delta(2, "soft_blocks"), "soft_flips": delta(2, "soft_flips"),
              # a block that fails the three alignments runs the search: it ends corrected (either way) or bad
              "blocks_that_ran_the_search": round((delta(1, "corrected") + delta(1, "bad")) / max(blocks_soft, 1), 3)})
        dh.close()
        ds.close()
        torch.cuda.empty_cache()


class SoftStepper(TrackingStepper):
    """The metered, decoding, tracking stepper with the soft tracker call and the soft decoder."""

    def __init__(self, args, nch, first, local, nblocks):
        super().__init__(args, nch, first, local, nblocks)
        self.dec.close()
        self.dec = self.pkg.RdsDecoder(nch, device=local, soft_bits=6)

    def step(self, b, gather=None):
        bench.GpuStepper.step(self, b, gather)
        s = self.s_post
        s.wait_event(self.post_done[b])
        self.meter.audio(self.pipe, self.lr[b % 2], stream=s)
        self.meter.rds(self.pipe, stream=s)
        nbits, bits, soft = self.trk.feed(self.clean, stream=s, soft=True)
        self.dec.feed(nbits, bits, stream=s, soft=soft)
        self.post_done[b].record(s)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=5, help="interleaved repeats of every leg")
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r18" / "soft"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rds_soft: needs a GPU")
    pkg = bench._load_pkg()
    import real_time_sdr_amd.synth  # noqa: F401  (pkg.synth)
    out = pathlib.Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    lines = []

    def emit(d: dict) -> None:
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        (out / "bench_rds_soft.jsonl").write_text("\n".join(lines) + "\n")

    if not args.skip_calls:
        calls_alone(torch, pkg, np, args.channels, args.iters, args.repeat, emit)
    if not args.skip_pipeline:
        legs = (("decoding_track_clock", TrackingStepper), ("decoding_track_clock_soft", SoftStepper))
        got: dict = {n: [] for n, _ in legs}
        for rep in range(min(args.repeat, 3)):
            for name, factory in legs:
                r = bench_tuner.pipeline_step(args, factory, "4")
                got[name].append(r["ms_per_step"])
                emit({"leg": "pipeline_step", "name": name, "repeat": rep, "channels": args.channels, **r})
        med = {n: statistics.median(v) for n, v in got.items()}
        spread = {n: [min(v), max(v)] for n, v in got.items()}
        inside = bool(spread["decoding_track_clock_soft"][0] <= spread["decoding_track_clock"][1])
        emit({"leg": "pipeline_ratio", "median_ms": med, "spread_ms": spread,
              "soft_over_hard": round(med["decoding_track_clock_soft"] / med["decoding_track_clock"], 4),
              "added_us_per_step": round((med["decoding_track_clock_soft"] - med["decoding_track_clock"]) * 1e3, 2),
              "inside_spread": inside, "claim": "confirmed" if inside else "refuted"})


if __name__ == "__main__":
    main()
