#!/usr/bin/env python3
"""The limits of sdr_meter_rf_status's cnr_db, measured on the CPU model (tests/rf_model.py: the front end's own
taps, oracle.lpf(2.4e6, 1e5, 101), u8 input, mode 0); no GPU. For a carrier of amplitude 0.3 at OFFSET kHz from
the centre: what clean FM at 75 kHz deviation reads, and for true in-channel C/N of 0 .. 22 dB what an
unmodulated carrier and the FM signal read. Five blocks per signal, the last four in the run-long row.
The figures in include/sdr_amd.h and DESIGN.md 4d' come from `rf_limits.py 0` and `rf_limits.py 20`.
  python tools/rf_limits.py [OFFSET_KHZ]"""
from __future__ import annotations

import math
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
import oracle  # noqa: E402
import rf_model as rm  # noqa: E402

FS, NB, BLOCK_IQ, AMP = 2.4e6, 5, 73500, 0.3


def to_u8(z):
    q = np.empty(2 * z.size)
    q[0::2] = np.round(128 * z.real + 128)
    q[1::2] = np.round(128 * z.imag + 128)
    return np.clip(q, 0, 255).astype(np.uint8)


def reading(z) -> dict:
    ch = rm.EnvChannel(oracle, 0)
    rows = [rm.rf_row(ch.block(b)) for b in to_u8(z).reshape(NB, 2 * BLOCK_IQ)]
    return rm.status(rm.run_long(rows[1:]))


def main() -> None:
    off = float(sys.argv[1]) * 1e3 if len(sys.argv) > 1 else 0.0
    h = np.asarray(oracle.lpf(FS, 1e5, 101), np.float64)
    n = NB * BLOCK_IQ
    t = np.arange(n) / FS
    rng = np.random.default_rng(5)

    def fm(dev, tone):
        return AMP * np.exp(1j * (2 * np.pi * off * t + (dev / tone) * np.sin(2 * np.pi * tone * t)))

    for tone in (1e3, 15e3):
        st = reading(fm(75e3, tone))
        print("noise-free FM, 75 kHz deviation, %g Hz tone: cnr_db %.2f ripple %.2e" % (tone, st["cnr_db"], st["ripple"]))
    st = reading(fm(0.0, 1e3))
    print("noise-free carrier: cnr_db %.2f ripple %.2e" % (st["cnr_db"], st["ripple"]))
    gain = abs(np.sum(h * np.exp(-2j * np.pi * off * np.arange(h.size) / FS))) ** 2
    for want in range(0, 23, 2):
        nin = AMP * AMP * gain / 10 ** (want / 10) / float(np.sum(h * h))
        sigma = math.sqrt(max(nin - 2 / (12 * 128 * 128), 0) / 2)
        noise = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        true = rm.true_cnr_db(h, AMP, sigma, khz=off / 1e3)
        got = [reading(s + noise)["cnr_db"] - true for s in (fm(0.0, 1e3), fm(75e3, 1e3), fm(75e3, 15e3))]
        print("true C/N %5.2f dB: carrier %+.2f  FM 75 kHz / 1 kHz tone %+.2f  FM 75 kHz / 15 kHz tone %+.2f" % (true, *got))


if __name__ == "__main__":
    main()
