"""Child process of tests/test_gpu_multi_tuned.py (a process of its own, as bench.py's queue child:
the engine ends the process on a failure). Runs, on device-resident input:
  1. sdr_multi_run_tuned: the composite capture (1 row per block), 3 stations, captures of all three;
  2. sdr_multi_run, untuned, 3 channels, on the contexts the engine pooled after run 1;
  3. sdr_multi_run_tuned with a src out of range (refused before anything starts).
usage: tuner_multi_child.py COMPOSITE.npy PLAIN.npy OUT.npz CUS"""
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
    import tuner_model as tm
    pkg = load_pkg()
    comp_path, plain_path, out_path, cus = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    comp = torch.from_numpy(np.load(comp_path)).to(dev)       # [nb][1][bytes]
    plain = torch.from_numpy(np.load(plain_path)).to(dev)     # [nb][3][bytes]
    nb, nch = comp.shape[0], 3
    host = C.CDLL(str(ROOT / "real-time-sdr_amd" / "libsdr_host.so"))
    Opts, Stats = bench._multi_structs()
    host.sdr_multi_run.argtypes = [C.POINTER(Opts), C.POINTER(Stats)]
    host.sdr_multi_run_tuned.argtypes = [C.POINTER(Opts), C.POINTER(Tuning), C.POINTER(Stats)]
    info = pkg.Pipeline(1).info
    cap_ch = (C.c_int * nch)(0, 1, 2)

    def run(iq, tune):
        lr = np.zeros((nb, nch, 2 * info.n_audio), np.int16)
        nbits = np.zeros((nb, nch), np.int32)
        bits = np.zeros((nb, nch, pkg.SDR_MAX_BITS), np.uint8)
        o = Opts(nch=nch, mode=0, flags=0, device=0, pll_cus=cus, in_path=None, d_iq=iq.data_ptr(),
                 row_stride=iq.shape[2], block_stride=iq.shape[1] * iq.shape[2], nblocks=nb, out_prefix=None,
                 ncap=nch, cap_blocks=nb, cap_ch=cap_ch, cap_lr=lr.ctypes.data, cap_nbits=nbits.ctypes.data,
                 cap_bits=bits.ctypes.data, stamp_blocks=0, pll_end=None)
        st = Stats()
        torch.cuda.synchronize(dev)
        if tune is None:
            rc = host.sdr_multi_run(C.byref(o), C.byref(st))
        else:
            rc = host.sdr_multi_run_tuned(C.byref(o), C.byref(tune), C.byref(st))
        return rc, st, lr, nbits, bits

    src = (C.c_int32 * nch)(0, 0, 0)
    khz = (C.c_int32 * nch)(*tm.COMPOSITE_KHZ)
    rc1, st1, lr1, nbits1, bits1 = run(comp.contiguous(), Tuning(1, src, khz))
    rc2, st2, lr2, nbits2, bits2 = run(plain.contiguous(), None)
    bad = (C.c_int32 * nch)(0, 1, 0)                          # row 1 of a 1-row capture
    rc3 = run(comp.contiguous(), Tuning(1, bad, khz))[0]
    np.savez(out_path, lr1=lr1, nbits1=nbits1, bits1=bits1, lr2=lr2, nbits2=nbits2, bits2=bits2)
    print(json.dumps({"rc": [rc1, rc2, rc3], "blocks": [st1.blocks, st2.blocks],
                      "persistent": [st1.persistent, st2.persistent]}), flush=True)


if __name__ == "__main__":
    main()
