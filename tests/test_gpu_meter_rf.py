"""GPU: the IF envelope row of the exact front ends (SDR_FLAG_IF_ENVELOPE, sdr_frontend.hip) and the meter's RF
rows (sdr_meter_rf, k_meter_rf of sdr_meter.hip) against the CPU model of tests/rf_model.py. Every comparison is
bit for bit: floats as uint32, integers exactly."""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np
import pytest

import meter_model as mm
import rf_model as rm
import tuner_model as tm
from conftest import ROOT, channel_input

pytestmark = pytest.mark.gpu

NB = 3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_rows(got, want, what):
    bad = rm.same_rows(got, want)
    assert not bad, f"{what}: {bad}\n got  {got}\n want {want}"


def _mode_rows(synth, block_iq: int, nblocks: int) -> np.ndarray:
    """u8 [nblocks][3][2*block_iq]: two synthetic channels (the mode-0 sources' bytes, cut to the mode's block) and
    one of all-128 silence."""
    need = nblocks * 2 * block_iq
    have = -(-need // (2 * synth.BLOCK_IQ))
    rows = np.full((nblocks, 3, 2 * block_iq), 128, np.uint8)
    for c in (0, 1):
        rows[:, c] = channel_input(synth, c, have).reshape(-1)[:need].reshape(nblocks, 2 * block_iq)
    return rows


def _run(pkg, torch, mode, rows, flags, tuning=None, with_meter=True):
    """A context over rows u8 [nb][nrows][bytes] on the current stream: per block the front end, then the block's
    fm, its if_env (with the flag) and the meter's RF rows. tuning: (src, khz, nsrc)."""
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    nch = len(tuning[0]) if tuning else rows.shape[1]
    pipe = pkg.Pipeline(nch, mode=mode, flags=flags)
    if tuning:
        pipe.set_tuning(*tuning)
    env_on = bool(flags & pkg.IF_ENVELOPE)
    meter = pkg.Meter(nch, mode=mode) if env_on and with_meter else None
    out = {"fm": [], "env": [], "rf": []}
    for b in range(rows.shape[0]):
        if tuning:
            pipe.frontend_tuned(d[b])
        else:
            pipe.frontend(d[b])
        out["fm"].append(pipe.fm_demod().cpu().numpy())
        if env_on:
            out["env"].append(pipe.buffer("if_env").cpu().numpy())
        if meter:
            meter.rf(pipe)
            out["rf"].append(meter.read_rf())
    if meter:
        meter.close()
    pipe.close()
    return {k: np.stack(v) for k, v in out.items() if v}


def _model_untuned(oracle, mode, rows):
    """(env [nch][nb][n], RF rows [nch][nb]) of the model."""
    env = []
    for c in range(rows.shape[1]):
        ch = rm.EnvChannel(oracle, mode)
        env.append([ch.block(rows[b, c]) for b in range(rows.shape[0])])
    return np.asarray(env), np.asarray([[rm.rf_row(e) for e in ce] for ce in env])


# ---------------------------------------------------------------- untuned, every decimation
@pytest.fixture(scope="module")
def untuned0(pkg, oracle, synth, torch_cuda):
    """Mode 0: the bytes, the flagged context's run, and the model; shared and left unchanged."""
    rows = _mode_rows(synth, pkg.Pipeline(1, mode=0).info.block_iq, NB)
    got = _run(pkg, torch_cuda, 0, rows, pkg.IF_ENVELOPE)
    env, rf = _model_untuned(oracle, 0, rows)
    return {"rows": rows, "got": got, "env": env, "rf": rf}


def _check_untuned(pkg, torch, mode, rows, got, env, rf):
    nb, nch = rows.shape[0], rows.shape[1]
    plain = _run(pkg, torch, mode, rows, 0)
    assert got["env"].shape == (nb, nch, env.shape[2])
    for b in range(nb):
        for c in range(nch):
            assert np.array_equal(_u32(got["env"][b, c]), _u32(env[c][b])), f"mode {mode} if_env ch {c} block {b}"
            _assert_rows(got["rf"][b][c], rf[c][b], f"mode {mode} row ch {c} block {b}")
        assert np.array_equal(_u32(got["fm"][b]), _u32(plain["fm"][b])), f"mode {mode} fm block {b}"
    assert not got["env"][:, 2].any() and not np.signbit(got["env"][:, 2]).any()      # silence: +0 throughout
    assert got["env"][:, :2].min() >= 0 and got["rf"]["env_sum"][:, 0].min() > 0
    assert (got["rf"]["n"] == env.shape[2]).all() and (got["rf"]["flags"] == rm.ROW_RF).all()


def test_untuned_mode0(pkg, torch_cuda, untuned0):
    """k_frontend2<8, 10, false, true>: 7350 outputs over 15 tiles; block 0 from the zero state and carry, blocks 1
    and 2 from the tail and carry of either parity."""
    u = untuned0
    _check_untuned(pkg, torch_cuda, 0, u["rows"], u["got"], u["env"], u["rf"])


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_untuned_other_modes(pkg, oracle, synth, torch_cuda, mode):
    """Decimations 4, 10 and 3; rows of 13230, 8000 and 12800 outputs (none a multiple of the 511-output tile)."""
    rows = _mode_rows(synth, pkg.Pipeline(1, mode=mode).info.block_iq, NB)
    got = _run(pkg, torch_cuda, mode, rows, pkg.IF_ENVELOPE)
    env, rf = _model_untuned(oracle, mode, rows)
    _check_untuned(pkg, torch_cuda, mode, rows, got, env, rf)


# ---------------------------------------------------------------- tuned
TUNE = ([0, 0, 0, 1], [-600, 0, 500, 0], 2)


@pytest.fixture(scope="module")
def tuned0(pkg, oracle, synth, torch_cuda):
    """Mode 0: the tuner tests' composite capture and a silent row; the three stations and one channel on silence."""
    comp = tm.composite(synth)[0][:NB]
    rows = np.full((NB, 2, comp.shape[1]), 128, np.uint8)
    rows[:, 0] = comp
    got = _run(pkg, torch_cuda, 0, rows, pkg.IF_ENVELOPE, TUNE)
    fm, env = rm.run_tuned_env(pkg, oracle, 0, rows, TUNE[0], TUNE[1])
    return {"rows": rows, "got": got, "fm": fm, "env": env}


def test_tuned(pkg, torch_cuda, tuned0):
    """k_frontend_tuned<4, 10, false, true>: the mixer in front of the same FIR; 255-output tiles."""
    t = tuned0
    plain = _run(pkg, torch_cuda, 0, t["rows"], 0, TUNE)
    for b in range(NB):
        for c in range(4):
            what = f"ch {c} ({TUNE[1][c]} kHz) block {b}"
            assert np.array_equal(_u32(t["got"]["env"][b, c]), _u32(t["env"][c][b])), "if_env " + what
            assert np.array_equal(_u32(t["got"]["fm"][b, c]), _u32(t["fm"][c][b])), "fm " + what
            _assert_rows(t["got"]["rf"][b][c], rm.rf_row(t["env"][c][b]), "row " + what)
        assert np.array_equal(_u32(t["got"]["fm"][b]), _u32(plain["fm"][b])), f"fm against the unflagged context, block {b}"
    assert not t["got"]["env"][:, 3].any() and t["got"]["rf"]["env_max"][:, :3].min() > 0


# ---------------------------------------------------------------- PHASE_DEMOD | IF_ENVELOPE
def test_phase_demod_with_the_row(pkg, oracle, torch_cuda, untuned0, tuned0):
    """Both discriminators carry the row: the env row is that of the default discriminator's context, fm is the
    phase model's (k_frontend2<8, 10, true, true> and k_frontend_tuned<4, 10, true, true>)."""
    both = pkg.PHASE_DEMOD | pkg.IF_ENVELOPE
    u = untuned0
    got = _run(pkg, torch_cuda, 0, u["rows"], both)
    fm, env = rm.run_tuned_env(pkg, oracle, 0, u["rows"], [0, 1, 2], [0, 0, 0], phase=True)
    for b in range(NB):
        assert np.array_equal(_u32(got["env"][b]), _u32(u["got"]["env"][b])), f"untuned if_env block {b}"
        assert got["rf"][b].tobytes() == u["got"]["rf"][b].tobytes(), f"untuned rows block {b}"
        for c in range(3):
            assert np.array_equal(_u32(got["fm"][b, c]), _u32(fm[c][b])), f"untuned fm ch {c} block {b}"
            assert np.array_equal(_u32(env[c][b]), _u32(u["env"][c][b]))      # (the khz = 0 mixer changes nothing)
    assert not np.array_equal(_u32(got["fm"][:, 0]), _u32(u["got"]["fm"][:, 0]))
    t = tuned0
    got = _run(pkg, torch_cuda, 0, t["rows"], both, TUNE)
    fm, _ = rm.run_tuned_env(pkg, oracle, 0, t["rows"], TUNE[0], TUNE[1], phase=True)
    for b in range(NB):
        assert np.array_equal(_u32(got["env"][b]), _u32(t["got"]["env"][b])), f"tuned if_env block {b}"
        assert got["rf"][b].tobytes() == t["got"]["rf"][b].tobytes(), f"tuned rows block {b}"
        for c in range(4):
            assert np.array_equal(_u32(got["fm"][b, c]), _u32(fm[c][b])), f"tuned fm ch {c} block {b}"


# ---------------------------------------------------------------- the pipeline fill
def test_pre_parts_fill_the_same_row(pkg, torch_cuda, untuned0):
    """Block 0 through sdr_frontend_pre_parts in three parts (tile-range launches of the same kernel) gives the
    row, and the meter's rows, of the one whole-block launch; block 1 behind it continues from the same state."""
    torch = torch_cuda
    sys.path.insert(0, str(ROOT))
    import bench
    u = untuned0
    d = torch.from_numpy(u["rows"][:2]).cuda()
    nch, dev = 3, torch.device("cuda", 0)
    pipe = pkg.Pipeline(nch, flags=pkg.IF_ENVELOPE)
    meter = pkg.Meter(nch)
    cus = bench.pll_cus(nch, lambda n: pipe.plls_fits(n)["fits"])
    created: list[int] = []
    s_fe, s_pll, s_post, _ = bench.cu_masked_streams(torch, pkg, dev, str(cus), created)
    info = pipe.info
    lr = torch.empty(2, nch, 2 * info.n_audio, dtype=torch.int16, device=dev)
    clean = torch.empty(2, nch, info.n_rds, dtype=torch.float32, device=dev)
    rf = torch.zeros(2, nch * 32, dtype=torch.uint8, device=dev)
    env = torch.zeros(2, nch, info.block_if, dtype=torch.float32, device=dev)

    def copy_env(out, stream):
        """if_env of the current block into out on `stream`, without a synchronisation or an allocation (nothing
        in the loop may touch the null stream while the persistent launch waits for blocks)."""
        p, st, n = C.c_void_p(), C.c_size_t(), C.c_int()
        pkg.check(pkg.lib().sdr_ctx_buffer(pipe._h, b"if_env", C.byref(p), C.byref(st), C.byref(n)), "sdr_ctx_buffer")
        assert n.value == info.block_if
        rc = pkg._hip().hipMemcpy2DAsync(C.c_void_p(out.data_ptr()), C.c_size_t(4 * n.value), p, C.c_size_t(4 * st.value),
                                         C.c_size_t(4 * n.value), C.c_size_t(nch), C.c_int(3), C.c_void_p(stream.cuda_stream))
        assert rc == 0, rc

    pipe.plls_launch(2, stream=s_pll)
    for b in range(2):
        if b == 0:
            pipe.frontend_pre_parts(d[b], 3, stream=s_fe)
        else:
            pipe.frontend(d[b], stream=s_fe)
            pipe.pre(stream=s_fe)
            pipe.plls_signal(stream=s_fe)
        meter.rf(pipe, stream=s_fe)
        meter.rf_rows_into(rf[b], stream=s_fe)
        copy_env(env[b], s_fe)
        pipe.plls_wait(stream=s_post)
        pipe.stereo_post(lr[b], stream=s_post)
        pipe.rds_post(clean[b], bits=True, stream=s_post)
    torch.cuda.synchronize(dev)
    assert len(pipe.plls_report(stream=s_pll)) == 2
    rows = rf.cpu().numpy().view(rm.ROW_DTYPE).reshape(2, nch)
    env = env.cpu().numpy()
    meter.close()
    pipe.close()
    bench.destroy_masked_streams(torch, pkg, dev, created)
    for b in range(2):
        assert np.array_equal(_u32(env[b]), _u32(u["got"]["env"][b])), f"if_env block {b}"
        for c in range(nch):
            _assert_rows(rows[b][c], u["rf"][c][b], f"row ch {c} block {b}")


# ---------------------------------------------------------------- the meter's rows
def test_a_row_does_not_depend_on_the_batch(pkg, torch_cuda, untuned0):
    """Channel 1 alone at nch = 1 has the rows it has at nch = 3."""
    u = untuned0
    alone = _run(pkg, torch_cuda, 0, u["rows"][:, 1:2], pkg.IF_ENVELOPE)
    for b in range(NB):
        _assert_rows(alone["rf"][b][0], u["got"]["rf"][b][1], f"block {b}")
        assert np.array_equal(_u32(alone["env"][b, 0]), _u32(u["got"]["env"][b, 1]))


def test_the_64_byte_rows_are_untouched_and_reset_clears_both(pkg, torch_cuda, untuned0):
    """A run that also calls sdr_meter_rf writes the 64-byte rows of a run that does not; sdr_meter_reset zeroes
    both arrays."""
    torch = torch_cuda
    d = torch.from_numpy(untuned0["rows"]).cuda()

    def run(flags):
        pipe, meter = pkg.Pipeline(3, flags=flags), pkg.Meter(3)
        rows = []
        for b in range(NB):
            pipe.frontend(d[b])
            if flags:
                meter.rf(pipe)
            lr = pipe.stereo()
            pipe.rds()
            meter.audio(pipe, lr)
            meter.rds(pipe)
            rows.append(meter.rows())
        rf = meter.read_rf()
        meter.reset()
        assert not meter.rows().view(np.uint8).any() and not meter.read_rf().view(np.uint8).any()
        meter.close()
        pipe.close()
        return np.stack(rows), rf

    with_rf, rf = run(pkg.IF_ENVELOPE)
    without, none = run(0)
    assert with_rf.tobytes() == without.tobytes()
    assert not mm.same_rows(with_rf, without) and with_rf["fm_sq"][:, 0].min() > 0
    assert rf.tobytes() == untuned0["got"]["rf"][NB - 1].tobytes() and not none.view(np.uint8).any()


def test_rf_on_a_second_stream(pkg, oracle, synth, torch_cuda):
    """Five blocks, sdr_meter_rf and the copy of its rows on a second stream while the front end keeps running on
    the first, the host never waiting: the front end of block b + 2 waits for the reader of block b (REL_METER_RF),
    and every block's row equals the model."""
    torch = torch_cuda
    nb = 5
    rows = _mode_rows(synth, synth.BLOCK_IQ, nb)
    d = torch.from_numpy(rows).cuda()
    pipe, meter = pkg.Pipeline(3, flags=pkg.IF_ENVELOPE), pkg.Meter(3)
    s2 = torch.cuda.Stream()
    cap = torch.zeros(nb, 3 * 32, dtype=torch.uint8, device=d.device)
    for b in range(nb):
        pipe.frontend(d[b])
        ev = torch.cuda.Event()
        ev.record()
        s2.wait_event(ev)
        meter.rf(pipe, stream=s2)
        meter.rf_rows_into(cap[b], stream=s2)
    torch.cuda.synchronize()
    got = cap.cpu().numpy().view(rm.ROW_DTYPE).reshape(nb, 3)
    meter.close()
    pipe.close()
    _, rf = _model_untuned(oracle, 0, rows)
    for b in range(nb):
        for c in range(3):
            _assert_rows(got[b][c], rf[c][b], f"ch {c} block {b}")


# ---------------------------------------------------------------- refusals along the lifecycle
def test_lifecycle_refusals(pkg, torch_cuda, untuned0):
    torch = torch_cuda
    d = torch.from_numpy(untuned0["rows"]).cuda()
    pipe, meter = pkg.Pipeline(3, flags=pkg.IF_ENVELOPE), pkg.Meter(3)

    def refused(fn, *a, **k):
        before = meter.read_rf()
        with pytest.raises(pkg.SdrError) as e:
            fn(*a, **k)
        assert e.value.code == -1, e.value
        assert meter.read_rf().tobytes() == before.tobytes(), "a refused call touched the rows"

    assert not meter.read_rf().view(np.uint8).any()                 # zero after create
    refused(meter.rf, pipe)                                          # before any front end
    refused(pipe.buffer, "if_env")
    pipe.frontend(d[0])
    meter.rf(pipe)
    assert np.array_equal(_u32(pipe.buffer("if_env").cpu().numpy()), _u32(untuned0["got"]["env"][0]))
    first = meter.read_rf()
    assert first.tobytes() == untuned0["got"]["rf"][0].tobytes()
    fm = pipe.fm_demod()
    pipe.push_fm_demod(fm)                                           # a pushed block brings no I/Q
    refused(meter.rf, pipe)
    refused(pipe.buffer, "if_env")
    pipe.frontend(d[1])                                              # ... and the next front end has a row again
    meter.rf(pipe)
    assert meter.read_rf().tobytes() != first.tobytes()
    pipe.reset()
    refused(meter.rf, pipe)                                          # after sdr_ctx_reset: no front end yet
    refused(pipe.buffer, "if_env")
    pipe.frontend(d[0])
    meter.rf(pipe)
    assert meter.read_rf().tobytes() == first.tobytes()
    for other in (pkg.Pipeline(3), pkg.Pipeline(2, flags=pkg.IF_ENVELOPE), pkg.Pipeline(3, mode=2, flags=pkg.IF_ENVELOPE)):
        n = other.info.block_iq
        other.frontend(torch.full((other.nch, 2 * n), 128, dtype=torch.uint8, device=d.device))
        refused(meter.rf, other)                                     # no flag; another nch; another mode
        if not other.flags & pkg.IF_ENVELOPE:
            refused(other.buffer, "if_env")
        other.close()
    with pytest.raises(pkg.SdrError) as e:
        pkg.Pipeline(2, flags=pkg.FLAG_FAST_FRONTEND | pkg.IF_ENVELOPE)
    assert e.value.code == -1, e.value
    meter.close()
    pipe.close()
