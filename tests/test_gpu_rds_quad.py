"""GPU: the RDS chain's quadrature branch (include/sdr_amd.h: SDR_FLAG_RDS_QUAD, sdr_ctx_rds_clean_q; k_rds_mix_q
in sdr_kernels.hip) against the oracle's own primitives (tests/rds_quad_model.py), bit for bit in every block
from block 0, and against a context without the flag: everything else the context computes stays what it is.
The fused post stage and SDR_FLAG_KEEP_INTERMEDIATES, each with per-block sdr_plls and with one persistent
launch."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import rds_quad_model as qm

pytestmark = pytest.mark.gpu

NCH, NB = 3, 10


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def stations(synth, oracle):
    """(iq [NB][NCH][2 block_iq] u8, the model's rows per channel): computed once, read by every test."""
    iq = np.stack([np.stack([s.next_block() for _ in range(NB)]) for s in (synth.FMMultiplexSource(c) for c in range(NCH))],
                  axis=1)
    ref = [qm.run_channel(oracle, iq[:, c]) for c in range(NCH)]
    return iq, ref


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _run(pkg, torch, iq, flags: int, persistent: bool, nb: int = NB, pipe=None):
    """The blocks through a pipeline with per-block sdr_plls on one stream, or with one persistent launch on
    CU-masked streams; per block clean, clean_q (with the flag), bits, nbits, stereo, mono, and ipll's last sample
    and the quadrature intermediates of the last block."""
    quad = bool(flags & pkg.RDS_QUAD)
    d = torch.from_numpy(iq[:nb]).cuda()
    own = pipe is None
    pipe = pkg.Pipeline(NCH, flags=flags) if own else pipe
    info = pipe.info
    got = {k: [] for k in ("clean", "clean_q", "bits", "nbits", "stereo", "mono")}
    lr = [torch.empty(NCH, 2 * info.n_audio, dtype=torch.int16, device="cuda") for _ in range(2)]
    mono = torch.empty(NCH, info.n_audio, dtype=torch.int16, device="cuda")
    clean = torch.empty(NCH, info.n_rds, dtype=torch.float32, device="cuda")

    def keep(b, s):
        with torch.cuda.stream(s):
            got["stereo"].append(lr[b % 2].clone())
            got["clean"].append(clean.clone())
            got["bits"].append(pipe.bits.clone())
            got["nbits"].append(pipe.nbits.clone())
        if quad:
            got["clean_q"].append(pipe.rds_clean_q(stream=s))

    if not persistent:
        s = torch.cuda.current_stream()
        for b in range(nb):
            pipe.frontend(d[b])
            pipe.mono(mono)
            got["mono"].append(mono.clone())
            pipe.pre()
            pipe.plls()
            pipe.stereo_post(lr[b % 2])
            pipe.rds_post(clean, bits=True)
            keep(b, s)
        torch.cuda.synchronize()
        last = s
        handles = []
    else:
        L = pkg.lib()
        L.sdr_stream_create_cu_range.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]
        L.sdr_stream_destroy.argtypes = [C.c_void_p]
        handles = []
        for lo, n, exclude in ((0, 8, 0), (0, 8, 1), (0, 8, 1)):   # the PLLs on CUs [0, 8), the rest elsewhere
            h = C.c_void_p()
            assert L.sdr_stream_create_cu_range(C.byref(h), torch.cuda.current_device(), lo, n, exclude) == 0
            handles.append(h.value)
        s_pll, s_fe, s_post = (torch.cuda.ExternalStream(h) for h in handles)
        post = [torch.cuda.Event() for _ in range(nb)]
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.Stream()):    # nothing on the null stream while the launch waits
            pipe.plls_launch(nb, stream=s_pll)
            for b in range(nb):
                if b >= 2:
                    s_fe.wait_event(post[b - 2])
                pipe.frontend(d[b], stream=s_fe)
                pipe.mono(mono, stream=s_fe)
                with torch.cuda.stream(s_fe):
                    got["mono"].append(mono.clone())
                pipe.pre(stream=s_fe)
                pipe.plls_signal(stream=s_fe)
                pipe.plls_wait(stream=s_post)
                pipe.stereo_post(lr[b % 2], stream=s_post)
                pipe.rds_post(clean, bits=True, stream=s_post)
                keep(b, s_post)
                post[b].record(s_post)
            s_post.synchronize()
            s_fe.synchronize()
            assert len(pipe.plls_report(stream=s_pll)) == nb
        torch.cuda.synchronize()
        last = s_post
    got["ipll_last"] = pipe.buffer("ipll", stream=last).cpu().numpy()[:, -1].copy()
    if quad:
        got["dc_q"] = pipe.buffer("rds_dc_q", stream=last).cpu().numpy()
        got["filt_q"] = pipe.buffer("rds_filt_q", stream=last).cpu().numpy()
    out = {k: ([t.cpu().numpy() for t in v] if isinstance(v, list) else v) for k, v in got.items()}
    for h in handles:
        assert pkg.lib().sdr_stream_destroy(C.c_void_p(h)) == 0
    if own:
        pipe.close()
    return out


@pytest.mark.parametrize("persistent", [False, True], ids=["sdr_plls", "persistent"])
@pytest.mark.parametrize("keep", [False, True], ids=["fused", "keep_intermediates"])
def test_quadrature_rows_and_everything_else(pkg, torch_cuda, stations, keep, persistent):
    iq, ref = stations
    base = pkg.FLAG_KEEP_INTERMEDIATES if keep else 0
    plain = _run(pkg, torch_cuda, iq, base, persistent)
    quad = _run(pkg, torch_cuda, iq, base | pkg.RDS_QUAD, persistent)
    for b in range(NB):
        for c in range(NCH):
            assert np.array_equal(_u32(quad["clean_q"][b][c]), _u32(ref[c]["rds_clean_q"][b])), f"rds_clean_q block {b} ch {c}"
            # the reference chain beside it is the oracle's, and the context's without the flag
            assert np.array_equal(_u32(quad["clean"][b][c]), _u32(ref[c]["rds_clean"][b])), f"rds_clean block {b} ch {c}"
        for k in ("clean", "bits", "nbits", "stereo", "mono"):
            assert np.array_equal(quad[k][b].view(np.uint8), plain[k][b].view(np.uint8)), f"{k} block {b}"
    assert np.array_equal(_u32(quad["ipll_last"]), _u32(plain["ipll_last"]))
    for c in range(NCH):
        assert np.float32(quad["ipll_last"][c]).view(np.uint32) == np.float32(ref[c]["ipll_last"][-1]).view(np.uint32)
        assert np.array_equal(_u32(quad["dc_q"][c]), _u32(ref[c]["rds_dc_q"][-1])), f"rds_dc_q ch {c}"
        assert np.array_equal(_u32(quad["filt_q"][c]), _u32(ref[c]["rds_filt_q"][-1])), f"rds_filt_q ch {c}"
    # the rows are worth the test: both branches carry the subcarrier, at comparable power, and differ
    pi = float(np.mean(np.square(quad["clean"][-1][0]))), float(np.mean(np.square(quad["clean_q"][-1][0])))
    assert pi[0] > 0 and 0.25 < pi[1] / pi[0] < 4.0, pi


def test_reset_restarts_the_branch(pkg, torch_cuda, stations):
    iq, ref = stations
    pipe = pkg.Pipeline(NCH, flags=pkg.RDS_QUAD)
    first = _run(pkg, torch_cuda, iq, pkg.RDS_QUAD, False, nb=4, pipe=pipe)
    pipe.reset()
    again = _run(pkg, torch_cuda, iq, pkg.RDS_QUAD, False, nb=3, pipe=pipe)
    for b in range(3):
        for c in range(NCH):
            assert np.array_equal(_u32(again["clean_q"][b][c]), _u32(ref[c]["rds_clean_q"][b])), f"block {b} ch {c}"
            assert np.array_equal(_u32(first["clean_q"][b][c]), _u32(again["clean_q"][b][c]))
    pipe.close()


def test_the_flag_and_the_rows_are_refused_where_they_do_not_apply(pkg, torch_cuda):
    for kw in (dict(mode=1), dict(mode=2), dict(mode=3), dict(rds_on=False)):
        with pytest.raises(pkg.SdrError):
            pkg.Pipeline(NCH, flags=pkg.RDS_QUAD, **kw)
    pipe = pkg.Pipeline(NCH)
    for name in ("rds_clean_q", "rds_dc_q", "rds_filt_q"):
        with pytest.raises(pkg.SdrError):
            pipe.buffer(name)
    with pytest.raises(pkg.SdrError):
        pipe.rds_clean_q()
    pipe.close()
