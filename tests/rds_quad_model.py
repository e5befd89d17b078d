"""The RDS chain's quadrature branch (include/sdr_amd.h, SDR_FLAG_RDS_QUAD / sdr_ctx_rds_clean_q) out of the
oracle's own primitives: a second fmpll on gen_pilot with phaseAdjust -pi/2, a pllblock_args and a zeroed output
buffer of its own, then the reference's delay, mixer, 247/640 resampler and RRC with states of their own. It
reads the intermediates the oracle's rds block hands out (rds_band, gen_pilot) and the oracle channel's taps."""
from __future__ import annotations

import ctypes as C

import numpy as np

DELAY = 50              # the APF of rds.cpp:122: an exact 50-sample shift


def _taps(ptr: int, n: int) -> np.ndarray:
    return np.ctypeslib.as_array((C.c_float * n).from_address(ptr)).copy()


class QuadBranch:
    """One channel's quadrature branch beside an oracle.Channel(0, True)."""

    def __init__(self, oracle, chan):
        c = chan.state
        self.oracle = oracle
        self.n, self.if_Fs, T = c.block_if, c.if_Fs, c.rf_taps
        self.bb_h, self.rrc_h = _taps(c.rds_bb_h, c.rds_bb_ntaps), _taps(c.rrc_h, T)
        self.out_q = np.zeros(self.n + 1, np.float32)
        self.st = oracle.new_pll_state()
        self.hist = np.zeros(DELAY, np.float32)
        self.rs_state, self.rrc_state = np.zeros(T - 1, np.float32), np.zeros(T - 1, np.float32)

    def block(self, rds_band, gen_pilot) -> dict:
        """One block from the oracle's rds_band and gen_pilot rows: rds_dc_q, rds_filt_q, rds_clean_q, ipll_q."""
        o, n = self.oracle, self.n
        o.fmpll(gen_pilot, 114e3, self.if_Fs, self.out_q, self.st, 0.5, np.float32(-np.pi / 2), 0.001)
        delay = np.concatenate([self.hist, rds_band])[:n] + np.float32(0.0)
        self.hist = np.array(rds_band[-DELAY:], np.float32)
        dc = (np.float32(2.0) * delay) * self.out_q[:n]
        assert dc.dtype == np.float32
        filt = o.fir_resample(dc, self.bb_h, self.rs_state, 247, 640)
        clean = o.fir_decim(filt, self.rrc_h, self.rrc_state, 1)
        return {"rds_dc_q": dc, "rds_filt_q": filt, "rds_clean_q": clean, "ipll_q": self.out_q.copy()}


def run_channel(oracle, iq_blocks) -> dict:
    """The oracle's channel and the quadrature branch over iq_blocks: lists per block of rds_clean, rds_clean_q,
    rds_dc_q, rds_filt_q, bits (None before the reference decodes), mono, stereo and ipll's last sample."""
    oc = oracle.Channel(0, True)
    qb = QuadBranch(oracle, oc)
    out = {k: [] for k in ("rds_clean", "rds_clean_q", "rds_dc_q", "rds_filt_q", "bits", "mono", "stereo", "ipll_last")}
    for iq in iq_blocks:
        fm = oc.frontend(iq)
        out["mono"].append(oc.mono(fm))
        out["stereo"].append(oc.stereo(fm))
        r = oc.rds(fm, intermediates=True)
        q = qb.block(r["rds_band"], r["gen_pilot"])
        out["rds_clean"].append(r["rds_clean"])
        out["bits"].append(r["bits"])
        out["ipll_last"].append(r["ipll"][-1])
        for k in ("rds_clean_q", "rds_dc_q", "rds_filt_q"):
            out[k].append(q[k])
    return out
