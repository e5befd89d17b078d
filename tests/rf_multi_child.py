"""Child process of tests/test_gpu_multi_rf.py (a process of its own: the engine ends the process on a failure).
Runs sdr_multi_run_metered on device-resident input, four times, each writing its files under OUTDIR:
  plain_rf, plain   the untuned capture (nch rows per block) with and without SDR_FLAG_IF_ENVELOPE;
  tuned_rf, tuned   the shared capture (nsrc rows per block) under the tuning, with and without the flag.
usage: rf_multi_child.py PLAIN.npy TUNED.npy TUNE.json OUTDIR CUS"""
from __future__ import annotations

import ctypes as C
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


class Tuning(C.Structure):
    _fields_ = [("nsrc", C.c_int), ("src", C.POINTER(C.c_int32)), ("khz", C.POINTER(C.c_int32))]


def main() -> None:
    import torch
    import bench
    from conftest import load_pkg
    pkg = load_pkg()
    plain_path, tuned_path, tune_path, outdir, cus = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    plain = torch.from_numpy(np.load(plain_path)).to(dev).contiguous()     # [nb][nch][bytes]
    tuned = torch.from_numpy(np.load(tuned_path)).to(dev).contiguous()     # [nb][nsrc][bytes]
    tune = json.loads(pathlib.Path(tune_path).read_text())
    nch = len(tune["src"])
    assert plain.shape[1] == nch
    host = C.CDLL(str(ROOT / "real-time-sdr_amd" / "libsdr_host.so"))
    Opts, Stats = bench._multi_structs()
    host.sdr_multi_run_metered.argtypes = [C.POINTER(Opts), C.POINTER(Tuning), C.POINTER(pkg.MeterOpts), C.POINTER(Stats)]
    mo = pkg.meter_opts()
    t = Tuning(tune["nsrc"], (C.c_int32 * nch)(*tune["src"]), (C.c_int32 * nch)(*tune["khz"]))

    def run(iq, tp, flags, name):
        o = Opts(nch=nch, mode=0, flags=flags, device=0, pll_cus=cus, in_path=None, d_iq=iq.data_ptr(),
                 row_stride=iq.shape[2], block_stride=iq.shape[1] * iq.shape[2], nblocks=iq.shape[0],
                 out_prefix=str(pathlib.Path(outdir) / name).encode(), ncap=0, cap_blocks=0, cap_ch=None, cap_lr=None,
                 cap_nbits=None, cap_bits=None, stamp_blocks=0, pll_end=None)
        st = Stats()
        torch.cuda.synchronize(dev)
        rc = host.sdr_multi_run_metered(C.byref(o), tp, C.byref(mo), C.byref(st))
        return {"rc": rc, "blocks": st.blocks, "persistent": st.persistent}

    res = {"plain_rf": run(plain, None, pkg.IF_ENVELOPE, "plain_rf"), "plain": run(plain, None, 0, "plain"),
           "tuned_rf": run(tuned, C.byref(t), pkg.IF_ENVELOPE, "tuned_rf"), "tuned": run(tuned, C.byref(t), 0, "tuned")}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
