#!/usr/bin/env python3
"""Timing of the band scan (sdr_scan_block) in one process, mode 0, 128 capture rows (18.8 MB per block).

  1. Calls alone, by HIP events around `iters` back-to-back calls on one stream after a warm-up (each
     call reads another resident input block), interleaved over `repeat` rounds:
       sdr_scan_block           k_scan_psd + k_scan_accum
       sdr_hbm_copy             the same bytes through the calibration copy kernel: the byte floor
       sdr_frontend_tuned       1024 channels on those rows, which reads the same bytes (by events like
                                the others, and by the kernel's own workgroup stamps like
                                tools/bench_tuner.py)
     and the scan as a ratio to both.
  2. The tuned pipeline step on tools/bench_tuner.py's schedule (bench.run_rank, 1024 channels on 128
     rows), interleaved: with no scanner; with a Scanner.block per block on a further CU-masked stream
     over the non-PLL CUs; and with the Scanner.block on the front-end stream itself (no further
     hardware queue). The claim under test: a scan beside the pipeline does not lengthen the
     PLL-bound step.

Prints one JSON line per measurement and writes them to profiles/r08/scan/bench_scan.jsonl (--out).
  python tools/bench_scan.py [--channels 1024] [--rows 128] [--iters 200] [--repeat 5] [--steps 100] [--warmup 40]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import bench  # noqa: E402
import bench_tuner  # noqa: E402

WARM = 40


def timed(torch, stream, call, iters: int) -> float:
    """ms per call: events around iters back-to-back calls on `stream`."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for b in range(iters):
        call(b)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def calls_alone(torch, pkg, iq, nch: int, nsrc: int, iters: int, repeat: int, emit) -> None:
    dev = iq.device
    s = torch.cuda.Stream(dev)
    nb = iq.shape[0]
    scan = pkg.Scanner(0, nsrc)
    pipe = pkg.Pipeline(nch)
    pipe.set_tuning(*bench_tuner.tuning(nch, nsrc), nsrc)
    rows = [iq[b, :nsrc] for b in range(nb)]
    nbytes = nsrc * 2 * pipe.info.block_iq
    src = torch.empty(nb, (nbytes + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src[0])
    legs = {
        "sdr_scan_block": lambda b: scan.block(rows[b % nb], stream=s),
        "sdr_hbm_copy": lambda b: pkg.hbm_copy(dst, src[b % nb], stream=s),
        "sdr_frontend_tuned": lambda b: pipe.frontend_tuned(rows[b % nb], stream=s),
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
            emit({"leg": "call_alone", "call": name, "repeat": rep, "rows": nsrc, "iters": iters,
                  "channels": nch if name == "sdr_frontend_tuned" else None, "ms_per_call": round(ms, 4),
                  "input_MB": round(nbytes / 1e6, 1), "GBps_in": round(nbytes / ms / 1e6, 1)})
        scan.reset(stream=s)
    med = {k: statistics.median(v) for k, v in got.items()}
    seg = scan.segments_per_block
    n1, n2 = 48, 50
    macs = nsrc * seg * 2400 * (n1 + n2) * 4          # real multiply-adds of the two DFT passes
    emit({"leg": "call_alone_summary", "median_ms": {k: round(v, 4) for k, v in med.items()},
          "min_ms": {k: round(min(v), 4) for k, v in got.items()},
          "max_ms": {k: round(max(v), 4) for k, v in got.items()},
          "scan_over_copy": round(med["sdr_scan_block"] / med["sdr_hbm_copy"], 2),
          "scan_over_frontend_tuned": round(med["sdr_scan_block"] / med["sdr_frontend_tuned"], 2),
          "scan_real_GMAC": round(macs / 1e9, 2),
          "scan_TFMAps": round(macs / med["sdr_scan_block"] / 1e9, 2)})
    scan.close()
    pipe.close()
    del src, dst
    # the tuned kernel alone by its own stamps, as profiles/r07/tuner/ has it
    emit({"leg": "kernel_alone", **bench_tuner.kernel_alone(torch, pkg, iq, nch, nsrc, 50)})


def scan_stepper(nsrc: int, where: str):
    """bench_tuner's tuned stepper plus a Scanner.block per block: where = "masked" (its own stream over
    the non-PLL CUs) or "fe" (the front-end stream, after the block's front-end work)."""
    base = bench_tuner.tuned_stepper(nsrc)

    class ScanStepper(base):
        def __init__(self, args, nch, first, local, nblocks):
            super().__init__(args, nch, first, local, nblocks)
            self.scan = self.pkg.Scanner(0, nsrc, device=local)
            self.s_scan = self.s_fe
            if where == "masked":
                if self.cu_spec in ("", "0"):
                    raise RuntimeError("bench_scan: the masked leg needs CU-masked streams")
                L, h = self.pkg.lib(), C.c_void_p()
                rc = L.sdr_stream_create_cu_range(C.byref(h), self.dev.index, 0, int(self.cu_spec), 1)
                if rc != 0:
                    raise RuntimeError(f"sdr_stream_create_cu_range: {rc}")
                self.created.append(h.value)
                self.s_scan = self.torch.cuda.ExternalStream(h.value, device=self.dev)

        def step(self, b, gather=None):
            super().step(b, gather)
            self.scan.block(self.iq[b % self.ring][:nsrc], stream=self.s_scan)

        def close(self):
            self.torch.cuda.synchronize(self.dev)
            self.scan.close()
            super().close()
    return ScanStepper


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=5, help="interleaved repeats of every leg")
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r08" / "scan"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_scan: needs a GPU")
    pkg = bench._load_pkg()
    dev = torch.device("cuda", 0)
    out = pathlib.Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    lines = []

    def emit(d: dict) -> None:
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        (out / "bench_scan.jsonl").write_text("\n".join(lines) + "\n")

    iq = bench.make_input(torch, args.rows, 8, 0, dev)
    calls_alone(torch, pkg, iq, args.channels, args.rows, args.iters, args.repeat, emit)
    del iq
    torch.cuda.empty_cache()
    if not args.skip_pipeline:
        legs = (("tuned_no_scan", bench_tuner.tuned_stepper(args.rows)),
                ("tuned_scan_masked_stream", scan_stepper(args.rows, "masked")),
                ("tuned_scan_on_fe_stream", scan_stepper(args.rows, "fe")))
        got: dict = {n: [] for n, _ in legs}
        for rep in range(min(args.repeat, 3)):
            for name, factory in legs:
                r = bench_tuner.pipeline_step(args, factory, "1")
                got[name].append(r["ms_per_step"])
                emit({"leg": "pipeline_step", "name": name, "repeat": rep, "channels": args.channels,
                      "rows": args.rows, **r})
        med = {n: statistics.median(v) for n, v in got.items()}
        emit({"leg": "pipeline_ratio", "median_ms": med,
              "scan_masked_over_none": round(med["tuned_scan_masked_stream"] / med["tuned_no_scan"], 4),
              "scan_on_fe_over_none": round(med["tuned_scan_on_fe_stream"] / med["tuned_no_scan"], 4)})


if __name__ == "__main__":
    main()
