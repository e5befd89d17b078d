"""CPU models of the fast (int8 MFMA) front end, shared by tests/test_fast_fe_model.py and
tests/test_gpu_fast_frontend.py. Not a conftest.

Three things live here: truth() -- the f64 fm_demod of the definition; kernel_model() -- the
arithmetic of k_frontend_mfma / ft_tile_iq (real-time-sdr_amd/csrc/sdr_frontend.hip) and of the
tap digits (sdr_ctx.hip, "MFMA front end") restated in numpy, with five optional defects; tol() --
a per-sample bound on |kernel - truth| derived from that code, not measured.

Definition (rffrontend.cpp:58-71, filter.cpp:106-121, demod.cpp:3-24). x = (u8 - 128) / 128, the
taps h are the library's f32 taps oracle.lpf(rf_Fs, 1e5, 101) read as f64, and with the previous
block's last 100 samples as history (u8 128 before block 0)
    c[n] = sum_k h[k] x[D n - k]                    (I and Q alike; c = cI + i cQ)
    q[n] = (cI (cQ - pQ) - cQ (cI - pI)) / (cI^2 + cQ^2) = Im(c conj(p)) / |c|^2,   p[n] = c[n - 1],
q = 0 where cI = cQ = 0, p carried across blocks, p = (0, 0) before the first output. truth() sums
in f64 (a BLAS dot: its own error is below 101 2^-53 A, A = sum_k |h[k]| |x|, nine decimal orders
under everything below).

The kernel. F = 30 - ceil(log2 max|h|), H[k] = llround(h[k] 2^F), every H[k] in 4 balanced base-256
digits (digit 0 the most significant). Plane p of an output is P_p = sum_k digit_p(H[k]) m[D n - k]
with m = u8 - 128, exact in int32 (|P_p| <= 128 * 128 * 101 < 2^21). Then, u = 2^-24, ys = 2^-(F+7):
    hI = (P_0 << 8) + P_1,  lI = (P_2 << 8) + P_3        int32, exact; S = 65536 hI + lI = sum H m
    y  = fmaf((float)hI, ys * 65536, (float)lI * ys)     two conversions, two products, one fma in f32
                                                         (|lI| passes 2^24 readily, |hI| at full
                                                         scale where F = 33: the conversions round)
    num = cI * (cQ - qQ) - cQ * (cI - qI)                f32, five roundings, no contraction
    den = cI * cI + cQ * cQ                              f32, three roundings
    q   = num * rcp(den)                                 v_rcp_f32 (<= 1 ulp) and one rounding
    out = (cI == 0 & cQ == 0) ? +0 : q

The bound e on one component of y - c (E_COMPONENT below).
  * taps: |H[k] 2^-F - h[k]| <= 2^-(F+1), so |S ys - c| <= 2^-(F+1) X1, X1 = sum_k |x[D n - k]|
    over the 101 samples the taps meet (<= 101).                                           [e_q]
  * the line of ft_tile_iq is counted as it is written, for any f32 ys, one u per operation:
        t1 = (float)hI = hI (1 + d1),  k = ys * 65536.0f = 65536 ys (1 + d2),
        t2 = (float)lI * ys = lI ys (1 + d3)(1 + d4),  y = (t1 k + t2)(1 + d5),  |d| <= u,
    so |y - S ys| <= ((1 + u)^3 - 1)(|hI| 65536 ys + |lI| ys) <= 3u (1 + 2^-22)(|S ys| + 2 |lI| ys).
    With |S ys| <= |c| + e_q and |lI| <= 257 * max|P| <= 257 * 2^14 X1, i.e. |lI| ys <= 257 2^(7-F) X1:
        e_r = 3u (1 + 2^-22) (|c| + e_q + 2 * 257 2^(7-F) X1)                               [e_r]
    (The context passes ys = 2^-(F+7), a power of two, which makes d2 and d4 zero: the sharp count
    on the high half is 2u. The bound does not lean on that; it is the room the defect-free model
    keeps under it in tests/test_fast_fe_model.py.)
  e = e_q + e_r per component; for the complex samples e_c = hypot(e_I, e_Q), and the previous
  sample's bound e_p[n] = e_c[n - 1] (0 before the first output, where p = (0, 0) exactly).

The bound on q (tol()). Exactly, for c' = c + dc, p' = p + dp, |dc| <= e_c, |dp| <= e_p and
N = Im(c conj p), M = |c|^2:
    |dN| <= e_c |p| + e_p |c| + e_c e_p,   |dM| <= 2 e_c |c| + e_c^2,
    |N'/M' - N/M| = |dN - q dM| / M' <= (|dN| + |q| |dM|) / (|c|^2 - |dM|)                 [main]
whenever |c|^2 > |dM| (e_c < (sqrt 2 - 1)|c|); otherwise the sample is ill-posed and tol = inf. To
first order and with one e this is [e (|p| + |c|) + 2 |q| e |c|] / |c|^2. The f32 discriminator adds
    U_N B / |c|^2,  B = |cI| |cQ - pQ| + |cQ| |cI - pI|,  U_N = 4u: the two differences, the two
        products and the final subtraction are (1 + d)^3 on terms whose magnitudes sum to B, 3u to
        first order, the fourth u for the higher orders;
    U_Q |q|,  U_Q = 6u: den is (1 + d)^2 (two non-negative products, one sum) = 2u, v_rcp_f32 is
        within 1 ulp <= 2^-23 = 2u relative, the product num * rcp rounds once = 1u, the sixth u
        for the higher orders.
B, |q| and |c|^2 are taken at the f64 values while the kernel rounds at its own operands: B moves by
<= 3 e_c (|p| + |c|) (9u of [main] once multiplied by 3u / |c|^2), |q| by [main] (6u of it), and
1/|c|^2 by 2.4 e_c / |c| relative (<= 16u of [main] on the U_N term, since B / |c|^2 <= 1.5 (|p| + |c|) / |c|):
31u in all, and [main] is multiplied by 1 + 2^-18 > 1 + 31u (SECOND_ORDER).
Where every byte the taps meet is 128 (X1 = 0 on I and Q) both sides are +0 exactly and tol = 0.

For the f32 reference the same form holds with e replaced by the sequential f32 FIR's bound: each
of the 101 products rounds once and takes part in at most 100 additions, |y - c| <= ((1 + u)^101 - 1) A
<= 102 u A (E_ORACLE); its discriminator rounds num as above and the quotient once.

No constant here was fitted to a GPU result.
"""
from __future__ import annotations

import numpy as np

NTAPS = 101
HP = NTAPS - 1
FT_NB = 32                       # sdr_internal.h: 16-output blocks per wave tile
FT_ND = 4                        # digit planes
U = 2.0 ** -24                   # unit roundoff of f32
U_N = 4 * U                      # num: cI * (cQ - qQ) - cQ * (cI - qI)
U_Q = 6 * U                      # den, v_rcp_f32, num * rcp
SECOND_ORDER = 1.0 + 2.0 ** -18  # > 1 + 31u, see the docstring
DEFECTS = ("three_planes", "two_planes", "tap_shift", "carry", "prev0")
TAP_SHIFT_ROW, TAP_SHIFT_TAP = 5, 1   # the defect "tap_shift": row 5 of every 16, tap 1 reads h[0]


def adv(D: int) -> int:
    """ft_adv(D, FT_NB): outputs a wave tile writes."""
    return 16 * FT_NB - 8 if D == 3 else 16 * FT_NB - 4


def carry(D: int) -> int:
    """ft_carry(D): outputs a tile computes ahead of the first it writes."""
    return {10: 2, 4: 1, 3: 4}[D]


_GEOM: dict = {}


def geometry(oracle, mode: int) -> dict:
    """rf_Fs, D, block_iq, block_if and the f32 taps of a mode (the oracle's mode table and lpf)."""
    if mode not in _GEOM:
        ch = oracle.Channel(mode, True)
        st = ch.state
        g = {"fs": int(st.rf_Fs), "D": int(st.rf_decim), "block_iq": int(ch.block_iq), "block_if": int(ch.block_if)}
        g["h"] = oracle.lpf(float(g["fs"]), 1e5, NTAPS)
        assert g["block_iq"] == g["D"] * g["block_if"] and g["h"].dtype == np.float32
        _GEOM[mode] = g
    return _GEOM[mode]


def tap_digits(h: np.ndarray):
    """(F, H, dig): sdr_ctx.hip's fixed-point taps. H int64 [101], dig int64 [101][4], digit 0 the most
    significant, every digit in [-128, 127] and sum_p dig[k][p] 256^(3-p) = H[k]."""
    h64 = h.astype(np.float64)
    F = 8 * FT_ND - 2 - int(np.ceil(np.log2(np.abs(h64).max())))
    v = h64 * 2.0 ** F                                                  # exact: a power-of-two scaling
    H = (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)       # llround: halves away from zero
    dig = np.zeros((NTAPS, FT_ND), np.int64)
    q = H.copy()
    for p in range(FT_ND - 1, -1, -1):
        d = np.mod(q, 256)
        d = np.where(d >= 128, d - 256, d)
        dig[:, p] = d
        q = (q - d) // 256
    assert np.all(q == 0) and np.all(np.abs(dig) <= 128) and np.all(dig <= 127)
    assert np.array_equal(((dig[:, 0] * 256 + dig[:, 1]) * 256 + dig[:, 2]) * 256 + dig[:, 3], H)
    return F, H, dig


def _components(rows_u8: np.ndarray, ch: int):
    """m = u8 - 128 of one channel's whole run as two f64 streams (I, Q), 100 zeros of history first."""
    s = np.concatenate([np.full(2 * HP, 128, np.uint8), np.ascontiguousarray(rows_u8[:, ch, :]).reshape(-1)])
    m = s.astype(np.float64) - 128.0
    return np.ascontiguousarray(m[0::2]), np.ascontiguousarray(m[1::2])


def _windows(v: np.ndarray, D: int, n: int) -> np.ndarray:
    """[n][101] view: row g holds m[D g - 100 + s], s = 0..100, which meets tap 100 - s."""
    assert v.ndim == 1 and v.flags.c_contiguous and D * (n - 1) + NTAPS <= v.size
    return np.lib.stride_tricks.as_strided(v, (n, NTAPS), (D * v.itemsize, v.itemsize), writeable=False)


def _shape(a: np.ndarray, nb: int) -> np.ndarray:
    return a.reshape(nb, -1)


def truth(mode: int, rows_u8: np.ndarray, oracle) -> dict:
    """rows_u8: u8 [nblocks][nch][2*block_iq]. Returns f64 arrays [nblocks][nch][block_if]: q (fm_demod of
    the definition), cI, cQ, pI, pQ, AI, AQ (sum_k |h[k]| |x|) and XI, XQ (sum_k |x|), plus F and D."""
    g = geometry(oracle, mode)
    D, nif = g["D"], g["block_if"]
    nb, nch = rows_u8.shape[0], rows_u8.shape[1]
    assert rows_u8.dtype == np.uint8 and rows_u8.shape[2] == 2 * g["block_iq"]
    hrev = g["h"].astype(np.float64)[::-1].copy()
    out = {k: np.zeros((nb, nch, nif)) for k in ("q", "cI", "cQ", "pI", "pQ", "AI", "AQ", "XI", "XQ")}
    for ch in range(nch):
        comp = {}
        for name, v in zip("IQ", _components(rows_u8, ch)):
            W = _windows(v, D, nb * nif)
            comp[name] = ((W @ hrev) / 128.0, (np.abs(W) @ np.abs(hrev)) / 128.0, np.abs(W).sum(axis=1) / 128.0)
        cI, cQ = comp["I"][0], comp["Q"][0]
        pI, pQ = np.concatenate([[0.0], cI[:-1]]), np.concatenate([[0.0], cQ[:-1]])
        den = cI * cI + cQ * cQ
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(den == 0.0, 0.0, (cI * (cQ - pQ) - cQ * (cI - pI)) / den)
        for k, a in (("q", q), ("cI", cI), ("cQ", cQ), ("pI", pI), ("pQ", pQ), ("AI", comp["I"][1]),
                     ("AQ", comp["Q"][1]), ("XI", comp["I"][2]), ("XQ", comp["Q"][2])):
            out[k][:, ch, :] = _shape(a, nb)
    out["F"], out["D"] = tap_digits(g["h"])[0], D
    return out


def kernel_model(mode: int, rows_u8: np.ndarray, oracle, defect: str | None = None, margins: dict | None = None):
    """fm_demod of k_frontend_mfma restated: f32 [nblocks][nch][block_if]. defect: None or one of DEFECTS.
    margins (a dict) receives the largest |plane sum|, |hI| = |(a0 << 8) + a1| and |lI| = |(a2 << 8) + a3| met,
    as "plane", "pair" and "pair_lo"."""
    assert defect is None or defect in DEFECTS
    g = geometry(oracle, mode)
    D, nif = g["D"], g["block_if"]
    nb, nch = rows_u8.shape[0], rows_u8.shape[1]
    F, H, dig = tap_digits(g["h"])
    digrev = dig[::-1].astype(np.float64).copy()          # row s meets tap 100 - s
    ys = np.float32(2.0 ** -(F + 7))
    ADV, CARRY = adv(D), carry(D)
    n = np.arange(nb * nif) % nif                          # output index within its block
    row16 = (n - ((n // ADV) * ADV - CARRY)) % 16          # row within the 16-output MFMA block of its tile
    fm = np.zeros((nb, nch, nif), np.float32)
    worst_plane = worst_pair = worst_lo = 0
    for ch in range(nch):
        y = []
        for v in _components(rows_u8, ch):
            W = _windows(v, D, nb * nif)
            P = W @ digrev                                 # f64, exact: integers below 2^21
            if defect == "tap_shift":                      # A[i][k] = digit(h[D i + 99 - k]) at one (row, tap)
                hit = row16 == TAP_SHIFT_ROW
                P[hit] += np.outer(W[hit, HP - TAP_SHIFT_TAP], (dig[TAP_SHIFT_TAP - 1] - dig[TAP_SHIFT_TAP]))
            P = P.astype(np.int64)
            if defect == "three_planes":
                P[:, 3] = 0
            elif defect == "two_planes":
                P[:, 2:] = 0
            hI, lI = (P[:, 0] << 8) + P[:, 1], (P[:, 2] << 8) + P[:, 3]
            worst_plane = max(worst_plane, int(np.abs(P).max()))
            worst_pair, worst_lo = max(worst_pair, int(np.abs(hI).max())), max(worst_lo, int(np.abs(lI).max()))
            assert max(worst_plane, worst_pair, worst_lo) < 2 ** 31, "an int32 of ft_tile_iq would overflow"
            # fmaf((float)hI, ys * 65536, (float)lI * ys): both products are exact, so the fma is the one
            # rounding of (fl(hI) * 65536 + fl(lI)) * ys; the integer is below 2^48 and its conversion rounds once
            T = hI.astype(np.float32).astype(np.int64) * 65536 + lI.astype(np.float32).astype(np.int64)
            y.append(T.astype(np.float32) * ys)
        cI, cQ = y
        pI, pQ = np.concatenate([[np.float32(0)], cI[:-1]]), np.concatenate([[np.float32(0)], cQ[:-1]])
        if defect == "carry":                              # row 0 of a 16-row block: row 14, not row 15, before it
            hit = (row16 == 0) & (np.arange(nb * nif) >= 2)
            pI[hit], pQ[hit] = cI[np.nonzero(hit)[0] - 2], cQ[np.nonzero(hit)[0] - 2]
        elif defect == "prev0":                            # output 0 of each block: (0, 0), not prev_in
            pI[n == 0], pQ[n == 0] = 0.0, 0.0
        assert all(a.dtype == np.float32 for a in (cI, cQ, pI, pQ))
        with np.errstate(all="ignore"):
            num = cI * (cQ - pQ) - cQ * (cI - pI)
            den = cI * cI + cQ * cQ
            q = num * (np.float32(1.0) / den)
        assert q.dtype == np.float32
        fm[:, ch, :] = _shape(np.where((cI == 0) & (cQ == 0), np.float32(0.0), q), nb)
    if margins is not None:
        margins["plane"] = max(margins.get("plane", 0), worst_plane)
        margins["pair"] = max(margins.get("pair", 0), worst_pair)
        margins["pair_lo"] = max(margins.get("pair_lo", 0), worst_lo)
    return fm


def _prev(e: np.ndarray) -> np.ndarray:
    """e of the previous output along the run ([nblocks][nch][block_if]); 0 before the first."""
    nb, nch, nif = e.shape
    s = e.transpose(1, 0, 2).reshape(nch, nb * nif)
    s = np.concatenate([np.zeros((nch, 1)), s[:, :-1]], axis=1)
    return s.reshape(nch, nb, nif).transpose(1, 0, 2)


def E_COMPONENT(c, X1, F):
    """The kernel's bound on one component of y - c (docstring: e_q + e_r)."""
    e_q = 2.0 ** -(F + 1) * X1                                                  # H[k] = llround(h[k] 2^F)
    # (float)hI | ys * 65536.0f | fmaf on the high half, (float)lI | * ys | fmaf on the low half
    e_r = 3 * U * (1 + 2.0 ** -22) * (np.abs(c) + e_q + 2 * 257 * 2.0 ** (7 - F) * X1)
    return e_q + e_r


def E_ORACLE(A):
    """The sequential f32 FIR's bound on one component (filter.cpp:110-116)."""
    return 102 * U * A


def tol(t: dict, reference: bool = False) -> np.ndarray:
    """Per-sample bound on |fm_demod - t["q"]|, [nblocks][nch][block_if]: of the MFMA kernel, or with
    reference=True of the f32 reference. inf where the sample is ill-posed, 0 where the taps meet only
    u8 128 (both sides are +0 there)."""
    cI, cQ, pI, pQ, q = t["cI"], t["cQ"], t["pI"], t["pQ"], np.abs(t["q"])
    if reference:
        eI, eQ = E_ORACLE(t["AI"]), E_ORACLE(t["AQ"])
    else:
        eI, eQ = E_COMPONENT(cI, t["XI"], t["F"]), E_COMPONENT(cQ, t["XQ"], t["F"])
    ec = np.hypot(eI, eQ)
    ep = _prev(ec)
    ac, ap = np.hypot(cI, cQ), np.hypot(pI, pQ)
    dN = ec * ap + ep * ac + ec * ep
    dM = 2 * ec * ac + ec * ec
    M = ac * ac
    B = np.abs(cI) * np.abs(cQ - pQ) + np.abs(cQ) * np.abs(cI - pI)
    with np.errstate(divide="ignore", invalid="ignore"):
        main = np.where(M > dM, (dN + q * dM) / (M - dM), np.inf)
        out = np.where(M > dM, main * SECOND_ORDER + U_Q * q + U_N * B / M, np.inf)
    return np.where((t["XI"] == 0) & (t["XQ"] == 0), 0.0, out)


def ratio(got: np.ndarray, t: dict, tolerance: np.ndarray) -> np.ndarray:
    """|got - t["q"]| / tolerance per sample: 0 where the error is 0 or the sample ill-posed (tolerance inf),
    inf where an error meets a tolerance of 0."""
    err = np.abs(got.astype(np.float64) - t["q"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((err == 0) | np.isinf(tolerance), 0.0, err / tolerance)


def rows_of(t: dict, j: int) -> dict:
    """truth() restricted to channel j (still [nblocks][1][block_if])."""
    return {k: (v[:, j:j + 1] if isinstance(v, np.ndarray) else v) for k, v in t.items()}


# ------------------------------------------------------------------------------------------------
# Inputs shared by the CPU and the GPU test
# ------------------------------------------------------------------------------------------------
EXTREME_ROWS = ("all_0", "all_255", "alternating", "window_mid", "window_straddle", "window_tile")


def extreme_outputs(oracle, mode: int) -> dict:
    """The run-wide output index (block * block_if + n) whose taps each window row's window meets: the middle
    of block 0, an output of block 1 whose window begins in block 0 (the tail path), and output ADV of
    block 0, the first a second tile writes."""
    g = geometry(oracle, mode)
    D, nif = g["D"], g["block_if"]
    return {"window_mid": nif // 2 + 3, "window_straddle": nif + (50 + D - 1) // D, "window_tile": adv(D)}


def extremes(oracle, mode: int, nblocks: int = 3) -> np.ndarray:
    """u8 [nblocks][6][2*block_iq], rows as EXTREME_ROWS: every byte 0 (int8 -128 on every operand), every
    byte 255, samples alternating (0, 0) and (255, 255), and three rows of u8 128 with one full-scale
    window each, whose I byte is 255 where the tap it meets is positive and 0 elsewhere and whose Q byte is
    the opposite: |y| there is the largest the taps allow."""
    g = geometry(oracle, mode)
    D, niq = g["D"], g["block_iq"]
    s = np.full((len(EXTREME_ROWS), nblocks * niq, 2), 128, np.uint8)
    s[0], s[1] = 0, 255
    s[2, 0::2], s[2, 1::2] = 0, 255
    pos = g["h"] > 0
    for name, out in extreme_outputs(oracle, mode).items():
        r = EXTREME_ROWS.index(name)
        idx = D * out - np.arange(NTAPS)                    # tap k meets sample D out - k of the run
        assert idx.min() >= 0 and idx.max() < nblocks * niq
        s[r, idx, 0] = np.where(pos, 255, 0)
        s[r, idx, 1] = np.where(pos, 0, 255)
    return np.ascontiguousarray(s.reshape(len(EXTREME_ROWS), nblocks, 2 * niq).transpose(1, 0, 2))


def steady_from(D: int) -> int:
    """First output of block 0 whose window and whose previous output's window have left the u8-128 history."""
    return (HP + D - 1) // D + 1
