"""GPU parity of the batched primitives (include/sdr_amd.h) at the shapes, states and values
tests/test_gpu_primitives.py does not reach: many lanes and carried state for the Manchester and
differential decoders, the empty row the library defines, every sps / n edge and the non-finite rule of
sdr_cdr, long and short FIR states, resampler shapes with U > D and tap-less phases, the polyphase cache's
eviction, and tiny / huge / zero samples at the block edges of the reference discriminator.

Every comparison is exact (f32 as uint32) against the oracle's C port, or against tests/prim_model.py
where the reference's C is undefined. Every output buffer is wider than needed and pre-filled with a
sentinel that must survive wherever the definition writes nothing."""
from __future__ import annotations

import numpy as np
import pytest

import prim_model as pm

pytestmark = pytest.mark.gpu

F_SENT = np.float32(-777.25)      # sentinel of f32 outputs
B_SENT = 0xEE                     # sentinel of byte outputs
SYM_PAD = 0xA5                    # padding of symbol rows


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _padded(torch, a, stride, fill):
    """Device tensor [rows][stride] filled with `fill`, holding `a` in its first columns; returns
    (whole tensor, the [rows][a.shape[1]] view a primitive is given)."""
    a = np.ascontiguousarray(a)
    t = torch.full((a.shape[0], stride), fill, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    v = t[:, :a.shape[1]]
    if a.shape[1]:
        v.copy_(torch.from_numpy(a))
    return t, v


def _state(torch, init, extra=8):
    """Contiguous [nch][nstate] state at the front of a wider, sentinel-filled allocation."""
    nch, ns = init.shape
    flat = torch.full((nch * ns + extra,), float(F_SENT), dtype=torch.float32, device="cuda")
    v = flat[:nch * ns].view(nch, ns)
    v.copy_(torch.from_numpy(init))
    return flat, v


def _sentinel_ok(whole, ncols):
    """The columns from ncols on of a [rows][stride] f32 array still hold the sentinel."""
    return np.array_equal(_u32(whole[:, ncols:]), np.full(whole[:, ncols:].shape, _u32([F_SENT])[0], np.uint32))


# ---------------------------------------------------------------- a. Manchester + differential chain
MAN_NCH, MAN_SYM_STRIDE, MAN_BITS_STRIDE, MAN_OUT_STRIDE = 130, 144, 72, 80
MAN_BLOCK_COUNTS = (0, 1, 2, 3, 0)
MAN_COUNTS = (2, 3, 4, 5, 100, 101, 139, 140)


def _manchester_inputs():
    rng = np.random.default_rng(2024)
    ncall = len(MAN_BLOCK_COUNTS)
    counts = rng.choice(MAN_COUNTS, (ncall, MAN_NCH))
    counts[:, 1] = rng.choice([3, 5, 101, 139], ncall)          # odd counts in every call
    counts[:, 5] = (3, 0, 0, 5, 4)                               # a pending half symbol through two empty calls
    counts[:, 7] = (4, 0, 1, 1, 2)
    streams = []
    for ch in range(MAN_NCH):
        total = int(counts[:, ch].sum())
        if ch % 2 == 0:      # a valid biphase stream (pairs 01 / 10) cut at an odd position
            b = rng.integers(0, 2, total // 2 + 2)
            s = np.stack([b, 1 - b], axis=1).reshape(-1)[1:1 + total]
        else:
            s = rng.integers(0, 2, total)
        streams.append(s.astype(np.int32))
    streams[3][:] = 0                                            # score 0: start = 0
    streams[5][:3] = (0, 1, 1)                                   # score +1: start 0, bit 0, half symbol 1 pending
    streams[7][:4] = (0, 0, 1, 1)                                # score -1: start 1, bit 0, half symbol 1 pending
    return counts, streams


def test_manchester_differential_chain(pkg, oracle, torch_cuda):
    """130 channels (two full groups of 64 lanes and one of 2), five calls with block_count = block_num =
    0, 1, 2, 3, 0, per-channel counts redrawn per call, padded rows. nbits, bits, {half_symbol, start},
    the differential output and last_bit equal the oracle's chain after every call; bytes past nbits keep
    the sentinel. Channels 5 and 7 have empty calls with a half symbol pending: the library's rule
    (nbits = 0, state, last_bit and rows untouched), for which the reference is undefined and the oracle
    is not called."""
    torch = torch_cuda
    counts, streams = _manchester_inputs()
    nch = MAN_NCH
    d_state = torch.zeros(nch, 2, dtype=torch.int32, device="cuda")
    # last_bit starts at random 0/1: block_num = 0 must ignore it in the first call already
    r_last = [int(v) for v in np.random.default_rng(7).integers(0, 2, nch)]
    d_last = torch.tensor(r_last, dtype=torch.int32).cuda()
    r_state = [[0, 0] for _ in range(nch)]
    pos = [0] * nch
    empties = 0
    for call, bc in enumerate(MAN_BLOCK_COUNTS):
        sym = np.full((nch, MAN_SYM_STRIDE), SYM_PAD, np.uint8)
        rows = []
        for ch in range(nch):
            m = int(counts[call, ch])
            rows.append(streams[ch][pos[ch]:pos[ch] + m])
            sym[ch, :m] = rows[ch]
            pos[ch] += m
        d_sym = torch.from_numpy(sym).cuda()
        d_nsym = torch.from_numpy(counts[call].astype(np.int32)).cuda()
        d_nbits = torch.full((nch + 6,), -9, dtype=torch.int32, device="cuda")
        d_bits = torch.full((nch, MAN_BITS_STRIDE), B_SENT, dtype=torch.uint8, device="cuda")
        d_out = torch.full((nch, MAN_OUT_STRIDE), B_SENT, dtype=torch.uint8, device="cuda")
        pkg.manchester_decode(d_bits, d_nbits[:nch], d_sym, d_nsym, bc, d_state)
        pkg.differential_decode(d_out, d_bits, d_nbits[:nch], bc, d_last)
        nbits, bits, out = d_nbits.cpu().numpy(), d_bits.cpu().numpy(), d_out.cpu().numpy()
        state, last = d_state.cpu().numpy(), d_last.cpu().numpy()
        assert np.all(nbits[nch:] == -9), f"call {call}: nbits written past nch"

        want = {}
        for ch in range(nch):
            m = int(counts[call, ch])
            if m == 0:                       # the library's rule; the previous state is the expectation
                assert r_state[ch][1] == 1, "the empty row is meant to meet a pending half symbol"
                want[ch] = (np.zeros(0, np.int32), np.zeros(0, np.int32))
                empties += 1
                continue
            before = list(r_state[ch])
            b = oracle.manchester(rows[ch], bc, r_state[ch])
            o, r_last[ch] = oracle.differential(b, bc, r_last[ch])
            want[ch] = (b, o)
            if call == 0 and ch % 2 == 0 and m >= 100:
                # (m - start) & 1 is the new start word: the search answered start = 1
                assert before == [0, 0] and (m ^ r_state[ch][1]) & 1 == 1, ch

        def check(ch):
            b, o = want[ch]
            nb = len(b)
            tag = f"call {call} (block_count {bc}) ch {ch} nsym {counts[call, ch]}"
            bad = []                         # every difference of the channel in one message
            if nbits[ch] != nb:
                bad.append(f"nbits {nbits[ch]} != {nb}")
            if not np.array_equal(bits[ch, :nb], b.astype(np.uint8)):
                bad.append("bits differ")
            if not np.all(bits[ch, nb:] == B_SENT):
                bad.append(f"bits row written past nbits: {[hex(v) for v in bits[ch, nb:nb + 4]]}")
            if [int(v) for v in state[ch]] != r_state[ch]:
                bad.append(f"state {[int(v) for v in state[ch]]} != {r_state[ch]}")
            if not np.array_equal(out[ch, :nb], o.astype(np.uint8)):
                bad.append("differential out differs")
            if not np.all(out[ch, nb:] == B_SENT):
                bad.append(f"out row written past nbits: {[hex(v) for v in out[ch, nb:nb + 4]]}")
            if last[ch] != r_last[ch]:
                bad.append(f"last_bit {last[ch]} != {r_last[ch]}")
            assert not bad, f"{tag}: " + "; ".join(bad)

        for ch in (1, 3, 5, 7, 63, 64, 128, 129):        # the designated channels and the group edges, by name
            check(ch)
        for ch in range(nch):
            check(ch)
    assert empties == 3


# ---------------------------------------------------------------- b. sdr_cdr
@pytest.mark.parametrize("sps,n", pm.CDR_CASES)
def test_cdr_edges(pkg, oracle, torch_cuda, sps, n):
    """67 rows at x_stride = n + 3: gaussian, all zero, all in (-1, 1), two equal maxima (the lower offset),
    the maximum at the last and at the first offset, +-3e6, and where n >= 2 * sps a NaN, two +Inf and
    +-3e9 (tests/prim_model.py). Every row against the header's integer model; every finite row against
    the oracle as well."""
    torch = torch_cuda
    x, kinds, want = pm.cdr_rows(sps, n)
    nch = x.shape[0]
    _, d_x = _padded(torch, x, n + 3, 7777.0)
    d_off = torch.full((nch + 5,), -7, dtype=torch.int32, device="cuda")
    pkg.cdr(d_off[:nch], d_x, sps)
    got = d_off.cpu().numpy()
    assert np.all(got[nch:] == -7)
    for r, finite in enumerate(pm.cdr_finite(kinds)):
        assert got[r] == pm.cdr_model(sps, x[r]), f"row {r} ({kinds[r]}): {got[r]} != model"
        if finite:
            assert got[r] == oracle.cdr(sps, x[r]), f"row {r} ({kinds[r]}): {got[r]} != oracle"
        if r in want:
            assert got[r] == want[r], f"row {r} ({kinds[r]}): {got[r]} != {want[r]}"


# ---------------------------------------------------------------- c. sdr_convolve_fir
FIR_TILE, FIR_LDS_MAX = 512, 160 * 1024       # csrc/sdr_internal.h, csrc/sdr_primitives.hip


def _fir_lds_bytes(ntaps, D, tile=FIR_TILE):
    return (((ntaps + 3) & ~3) + (tile - 1) * D + ntaps + 4) * 4


@pytest.mark.parametrize("nx,D,ntaps,nstate", [(5, 10, 101, 100), (37, 1, 600, 599), (1001, 3, 31, 64),
                                               (64, 1, 1, 1), (300, 7, 5, 4)])
def test_convolve_fir_edges(pkg, oracle, torch_cuda, nx, D, ntaps, nstate):
    """No output with a shifting state (nx < D), the chunked state shift (nx < nstate, nstate > 256),
    nstate > ntaps - 1, one tap, D > ntaps; three blocks, padded x and y rows, output and state after
    every block."""
    torch = torch_cuda
    rng = np.random.default_rng(nx * 31 + ntaps)
    nch, ny = 3, nx // D
    h = (rng.standard_normal(ntaps) * 0.05).astype(np.float32)
    st_ref = rng.standard_normal((nch, nstate)).astype(np.float32)
    flat, d_state = _state(torch, st_ref)
    d_h = torch.from_numpy(h).cuda()
    for blk in range(3):
        x = rng.standard_normal((nch, nx)).astype(np.float32)
        _, d_x = _padded(torch, x, nx + 5, 1e6)
        y_all = torch.full((nch, ny + 3), float(F_SENT), device="cuda")
        # (an empty view has no address: with no output the call gets the whole sentinel row)
        pkg.convolve_fir(y_all[:, :ny] if ny else y_all, d_x, d_h, d_state, D)
        y = y_all.cpu().numpy()
        st = d_state.cpu().numpy()
        for c in range(nch):
            ref = oracle.fir_decim(x[c], h, st_ref[c], D)
            assert np.array_equal(_u32(y[c, :ny]), _u32(ref)), f"block {blk} ch {c}: y"
            assert np.array_equal(_u32(st[c]), _u32(st_ref[c])), f"block {blk} ch {c}: state"
        assert _sentinel_ok(y, ny), f"block {blk}: y written past nx / D"
        assert np.all(_u32(flat[nch * nstate:].cpu().numpy()) == _u32([F_SENT])[0]), f"block {blk}: past the state"


def test_convolve_fir_refusals(pkg, torch_cuda):
    """nstate = ntaps - 2, and a (ntaps, D) whose tile does not fit the 160 KiB rule: -1, y and state as
    they were."""
    torch = torch_cuda
    rng = np.random.default_rng(77)
    nch = 3
    ntaps, D = 101, 1
    while _fir_lds_bytes(ntaps, D) <= FIR_LDS_MAX:
        D += 1
    assert _fir_lds_bytes(ntaps, D - 1) <= FIR_LDS_MAX < _fir_lds_bytes(ntaps, D)
    for nx, D_, ntaps_, nstate in ((200, 2, 31, 29), (2 * D, D, ntaps, ntaps - 1)):
        st0 = rng.standard_normal((nch, nstate)).astype(np.float32)
        _, d_state = _state(torch, st0)
        d_h = torch.from_numpy(rng.standard_normal(ntaps_).astype(np.float32)).cuda()
        d_x = torch.from_numpy(rng.standard_normal((nch, nx)).astype(np.float32)).cuda()
        d_y = torch.full((nch, nx // D_ + 3), float(F_SENT), device="cuda")
        with pytest.raises(pkg.SdrError) as e:
            pkg.convolve_fir(d_y[:, :nx // D_], d_x, d_h, d_state, D_)
        torch.cuda.synchronize()
        assert e.value.code == -1, e.value
        assert _sentinel_ok(d_y.cpu().numpy(), 0)
        assert np.array_equal(_u32(d_state.cpu().numpy()), _u32(st0))


# ---------------------------------------------------------------- d. sdr_convolve_fir_resample
def _resample_blocks(pkg, oracle, torch, rng, h, nx, U, D, nstate, nblocks, nch=3, tag=""):
    ny = nx * U // D
    st_ref = rng.standard_normal((nch, nstate)).astype(np.float32)
    flat, d_state = _state(torch, st_ref)
    d_h = torch.from_numpy(h).cuda()
    ys = []
    for blk in range(nblocks):
        x = rng.standard_normal((nch, nx)).astype(np.float32)
        _, d_x = _padded(torch, x, nx + 5, 1e6)
        y_all = torch.full((nch, ny + 3), float(F_SENT), device="cuda")
        pkg.convolve_fir_resample(y_all[:, :ny] if ny else y_all, d_x, d_h, d_state, U, D)
        y = y_all.cpu().numpy()
        st = d_state.cpu().numpy()
        for c in range(nch):
            ref = oracle.fir_resample(x[c], h, st_ref[c], U, D)
            assert np.array_equal(_u32(y[c, :ny]), _u32(ref)), f"{tag} block {blk} ch {c}: y"
            assert np.array_equal(_u32(st[c]), _u32(st_ref[c])), f"{tag} block {blk} ch {c}: state"
        assert _sentinel_ok(y, ny), f"{tag} block {blk}: y written past nx * U / D"
        assert np.all(_u32(flat[nch * nstate:].cpu().numpy()) == _u32([F_SENT])[0]), f"{tag}: past the state"
        ys.append(y[:, :ny])
    return ys


@pytest.mark.parametrize("nx,U,D,ntaps,nstate", [(100, 3, 2, 31, 10), (100, 7, 3, 5, 1), (50, 1, 60, 11, 10),
                                                 (8000, 147, 800, 14847, 150)])
def test_resample_edges(pkg, oracle, torch_cuda, nx, U, D, ntaps, nstate):
    """U > D (more outputs than inputs), ntaps < U (phases without a tap: exactly +0.0), no output at all,
    and nstate other than 100; three blocks, output and state after every block."""
    rng = np.random.default_rng(U * 1000 + D)
    h = (rng.standard_normal(ntaps) * 0.01).astype(np.float32)
    ys = _resample_blocks(pkg, oracle, torch_cuda, rng, h, nx, U, D, nstate, 3)
    if ntaps < U:
        n = np.arange(nx * U // D)
        empty = (n * D) % U >= ntaps
        assert empty.any() and not empty.all()
        for y in ys:
            assert np.all(_u32(y[:, empty]) == 0), "a phase without a tap is +0.0"


def test_resample_refusal(pkg, torch_cuda):
    """nstate = 99 below the look-back of 100 of (ntaps 14847, U 147): -1, y and state as they were."""
    torch = torch_cuda
    rng = np.random.default_rng(99)
    nch, nx, U, D, ntaps, nstate = 3, 8000, 147, 800, 14847, 99
    st0 = rng.standard_normal((nch, nstate)).astype(np.float32)
    _, d_state = _state(torch, st0)
    d_h = torch.from_numpy((rng.standard_normal(ntaps) * 0.01).astype(np.float32)).cuda()
    d_x = torch.from_numpy(rng.standard_normal((nch, nx)).astype(np.float32)).cuda()
    ny = nx * U // D
    d_y = torch.full((nch, ny + 3), float(F_SENT), device="cuda")
    with pytest.raises(pkg.SdrError) as e:
        pkg.convolve_fir_resample(d_y[:, :ny], d_x, d_h, d_state, U, D)
    torch.cuda.synchronize()
    assert e.value.code == -1, e.value
    assert _sentinel_ok(d_y.cpu().numpy(), 0)
    assert np.array_equal(_u32(d_state.cpu().numpy()), _u32(st0))


def test_resample_table_cache(pkg, oracle, torch_cuda):
    """20 distinct 8-tap filters (more than the 16 polyphase tables the process keeps, so at least one
    eviction whatever earlier tests left), each against the oracle; the first one again after its table
    was dropped; then the same taps under U = 2 and U = 3 (the key is (U, taps))."""
    rng = np.random.default_rng(1616)
    filters = [rng.standard_normal(8).astype(np.float32) for _ in range(20)]
    assert len({f.tobytes() for f in filters}) == 20
    for i, h in enumerate(filters + filters[:1]):
        _resample_blocks(pkg, oracle, torch_cuda, rng, h, 64, 2, 3, 5, 1, tag=f"filter {i}")
    for U in (2, 3, 2):
        _resample_blocks(pkg, oracle, torch_cuda, rng, filters[7], 64, U, 3, 5, 1, tag=f"U {U}")


# ---------------------------------------------------------------- e. sdr_fm_demod
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_fm_demod_edges(pkg, oracle, torch_cuda, n):
    """Around the 256-thread block edge, three blocks, padded rows. Row 0: unit variance with (0, 0) at the
    first and the last sample of block 1 (the zero branch, and prev = (0, 0) handed to block 2). Row 1:
    scaled by 1e-20 (a subnormal f32 numerator over an f64 denominator near 1e-40). Row 2: scaled by 3e19
    (I^2 + Q^2 overflows f32, not f64). Row 3: constant (numerator exactly 0). out and prev after every
    block.

    Row 2 is a phasor of nearly constant envelope with small phase steps, as an FM signal is: the f32
    numerator I * dQ - Q * dI then stays finite. With independent samples of that size both products
    overflow and their difference is inf - inf, a NaN whose sign bit is the host's choice, not the
    reference's."""
    torch = torch_cuda
    rng = np.random.default_rng(400 + n)
    nch = 4
    prev_ref = [np.zeros(2, np.float32) for _ in range(nch)]
    pflat = torch.full((nch * 2 + 6,), float(F_SENT), device="cuda")
    d_prev = pflat[:nch * 2].view(nch, 2)
    d_prev.zero_()
    phase = 0.1
    for blk in range(3):
        I = rng.standard_normal((nch, n)).astype(np.float32)
        Q = rng.standard_normal((nch, n)).astype(np.float32)
        if blk == 1:
            I[0, 0] = Q[0, 0] = 0.0
            I[0, n - 1] = Q[0, n - 1] = 0.0
        I[1] *= np.float32(1e-20)
        Q[1] *= np.float32(1e-20)
        ph = phase + np.cumsum(rng.uniform(-0.02, 0.02, n))
        amp = 3e19 * rng.uniform(0.99, 1.01, n)
        phase = ph[-1]
        I[2], Q[2] = (amp * np.cos(ph)).astype(np.float32), (amp * np.sin(ph)).astype(np.float32)
        I[3], Q[3] = 0.75, -1.25
        assert np.all(np.isfinite(I)) and np.all(np.isfinite(Q))
        with np.errstate(over="ignore"):
            assert np.all(np.isinf(I[2] * I[2] + Q[2] * Q[2]))      # overflows f32
        assert np.all(I[1] != 0) and np.all(np.abs(I[1]) < 1e-18)
        _, d_I = _padded(torch, I, n + 3, 5.0)
        _, d_Q = _padded(torch, Q, n + 3, 5.0)
        o_all = torch.full((nch, n + 5), float(F_SENT), device="cuda")
        pkg.fm_demod(o_all[:, :n], d_I, d_Q, d_prev)
        out = o_all.cpu().numpy()
        prev = d_prev.cpu().numpy()
        for c in range(nch):
            ref = oracle.fm_demod(I[c], Q[c], prev_ref[c])
            assert np.all(np.isfinite(ref)), f"block {blk} row {c}: the reference itself is not finite"
            assert np.array_equal(_u32(out[c, :n]), _u32(ref)), f"n {n} block {blk} row {c}: out"
            assert np.array_equal(_u32(prev[c]), _u32(prev_ref[c])), f"n {n} block {blk} row {c}: prev"
        if blk == 0 and n > 2:
            assert np.any(np.abs(out[1, :n]) > 0), "row 1 must not collapse to zero"
        assert _sentinel_ok(out, n), f"block {blk}: out written past n"
        assert np.all(_u32(pflat[nch * 2:].cpu().numpy()) == _u32([F_SENT])[0]), f"block {blk}: past prev"
