"""real-time-sdr_amd -- MI355X-native FM/RDS DSP hot path of TheZxc07/real-time-SDR.

Python binding (ctypes) of the C ABI in include/sdr_amd.h, implemented by libsdr_amd.so
(hand-written HIP kernels for gfx950). PyTorch is used only as device-memory / stream plumbing:
every call takes device pointers, and the torch helpers here just pass `tensor.data_ptr()` and
the current HIP stream. There is no CPU fallback: if the library cannot be loaded, every entry
point raises.

Reference interface mirrored (file:line in TheZxc07/real-time-SDR):
  convolveFIR (decimating)      src/filter.cpp:106-121   -> convolve_fir
  convolveFIR (resampling)      src/filter.cpp:123-147   -> convolve_fir_resample
  fmDemodNoArctan               src/demod.cpp:3-24       -> fm_demod
  fmpll / pllblock_args         src/pll.cpp:4-61         -> fmpll / PllState
  cdr                           src/rds_utilities.cpp:4-21 -> cdr
  RF_frontend / mono / stereo / rds stage bodies         -> Pipeline
"""
from __future__ import annotations

import ctypes as C
import os
import pathlib

HERE = pathlib.Path(__file__).resolve().parent
LIB_PATH = pathlib.Path(os.environ["SDR_AMD_LIB"]) if os.environ.get("SDR_AMD_LIB") else HERE / "libsdr_amd.so"  # override: A/B experiments (tools/)

SDR_OK = 0
SDR_E_TIMEOUT = -5           # a parity-release wait gave up: outputs poisoned until reset (include/sdr_amd.h)
SDR_MAX_SYMS = 256
SDR_MAX_BITS = 256
SDR_PCM_POISON = -32768      # audio of a block whose persistent PLL or release wait timed out (include/sdr_amd.h)
SDR_NBITS_POISONED = -2      # nbits of such a block (its rds_clean rows are NaN)
FLAG_FAST_FRONTEND = 0x1
FLAG_PLL_LIBM = 0x2
FLAG_KEEP_INTERMEDIATES = 0x4
PHASE_DEMOD = FLAG_PHASE_DEMOD = 0x8   # fm_demod is the phase step in radians (include/sdr_amd.h); not with FAST
RDS_QUAD = FLAG_RDS_QUAD = 0x10        # rds / rds_post also run the RDS chain's quadrature branch (Pipeline.rds_clean_q)
IF_ENVELOPE = FLAG_IF_ENVELOPE = 0x20  # the exact front ends keep the IF power row buffer("if_env") (Meter.rf); not with FAST

_lib = None


class SdrError(RuntimeError):
    def __init__(self, msg: str, code: int | None = None):
        super().__init__(msg)
        self.code = code


class PllState(C.Structure):
    """pllblock_args (include/pll.h:10-17); lastCarrier doubles as pllOut[last] (pll.cpp:18)."""
    _fields_ = [("feedbackI", C.c_float), ("feedbackQ", C.c_float), ("integrator", C.c_float),
                ("phaseEst", C.c_float), ("trigOffset", C.c_double), ("lastCarrier", C.c_float)]


class Info(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("nch", "mode", "rds_on", "rf_Fs", "rf_decim", "if_Fs", "audio_upsample",
                                        "audio_decim", "symbol_Fs", "rf_taps", "block_iq", "block_if", "n_audio",
                                        "n_rds", "history")]


class ScanOpts(C.Structure):
    """sdr_scan_opts (include/sdr_amd.h): the picker's options."""
    _fields_ = [(n, C.c_int) for n in ("half_width_khz", "step_khz", "first_khz", "sep_khz", "guard_khz")] + \
               [("thr_db", C.c_float)]


class MeterRow(C.Structure):
    """sdr_meter_row (include/sdr_amd.h): one channel's readings of one block, 64 bytes."""
    _fields_ = [(n, C.c_float) for n in ("fm_sum", "fm_sq", "fm_peak", "pilot_sq", "noise_sq", "rds_sq", "eye_abs",
                                          "eye_sq")] + \
               [(n, C.c_int32) for n in ("eye_n", "flags", "l_peak", "r_peak")] + \
               [(n, C.c_uint64) for n in ("l_sq", "r_sq")]


class MeterOpts(C.Structure):
    """sdr_meter_opts: the thresholds of meter_status."""
    _fields_ = [(n, C.c_float) for n in ("pilot_nr_min", "rds_nr_min", "offtune_min")] + [("silence_peak", C.c_int)]


class MeterState(C.Structure):
    """sdr_meter_state: what sdr_meter_status makes of a row."""
    _fields_ = [(n, C.c_double) for n in ("offset", "level_db", "pilot_nr", "rds_nr", "eye_db")] + [("flags", C.c_int)]


class MeterRfRow(C.Structure):
    """sdr_meter_rf_row (include/sdr_amd.h): one channel's IF envelope readings of one block, 32 bytes."""
    _fields_ = [(n, C.c_float) for n in ("env_sum", "env_sq", "env_min", "env_max")] + \
               [(n, C.c_int32) for n in ("n", "flags")] + [("reserved", C.c_int32 * 2)]


class MeterRfOpts(C.Structure):
    """sdr_meter_rf_opts: the threshold of meter_rf_status."""
    _fields_ = [("ripple_max", C.c_float)]


class MeterRfState(C.Structure):
    """sdr_meter_rf_state: what sdr_meter_rf_status makes of a row."""
    _fields_ = [(n, C.c_double) for n in ("level_dbfs", "ripple", "cnr_db", "fade_db", "crest_db")] + [("flags", C.c_int)]


class AudioOpts(C.Structure):
    """sdr_audio_opts: the de-emphasis time constant and the blend map's two pilot_nr corners."""
    _fields_ = [(n, C.c_float) for n in ("tau_us", "blend_lo", "blend_hi")]


class AudioState(C.Structure):
    """sdr_audio_state: one channel's filter state, current blend and gain and their targets, 24 bytes."""
    _fields_ = [("y", C.c_float * 2)] + [(n, C.c_float) for n in ("blend", "gain", "blend_target", "gain_target")]


class RdsGroup(C.Structure):
    """sdr_rds_group: one RDS group as the decoder emits it, 16 bytes."""
    _fields_ = [("w", C.c_uint16 * 4), ("ok", C.c_uint8), ("corrected", C.c_uint8), ("flags", C.c_uint8),
                ("reserved", C.c_uint8), ("bits", C.c_uint32)]


class RdsStats(C.Structure):
    """sdr_rds_stats: one channel's block and sync counters, 32 bytes."""
    _fields_ = [(n, C.c_uint32) for n in ("good", "corrected", "bad", "slips", "acquired", "lost", "groups", "synced")]


class RdsOpts(C.Structure):
    """sdr_rds_opts: the burst length the decoder corrects and the bad blocks in a row that end a sync."""
    _fields_ = [("max_burst", C.c_int), ("loss_blocks", C.c_int)]


class RdsStationC(C.Structure):
    """sdr_rds_station: the text layer's state of one station."""
    _fields_ = [("pi", C.c_uint16), ("pi_last", C.c_uint16), ("pi_valid", C.c_uint8), ("pi_seen", C.c_uint8),
                ("pty", C.c_uint8), ("tp", C.c_uint8), ("ta", C.c_uint8), ("ms", C.c_uint8), ("have_b", C.c_uint8),
                ("have_0", C.c_uint8), ("ps", C.c_uint8 * 8), ("ps_seen", C.c_uint8), ("ps_complete", C.c_uint8),
                ("ps_done", C.c_uint8 * 8), ("rt", C.c_uint8 * 64), ("rt_ab", C.c_uint8), ("rt_have_ab", C.c_uint8),
                ("rt_len", C.c_uint8), ("rt_seen", C.c_uint64), ("ct_valid", C.c_uint8), ("ct_hour", C.c_uint8),
                ("ct_minute", C.c_uint8), ("ct_month", C.c_uint8), ("ct_day", C.c_uint8), ("ct_offset", C.c_int8),
                ("ct_year", C.c_int32), ("ct_mjd", C.c_int32), ("af_n", C.c_uint8), ("af_expect", C.c_uint8),
                ("af", C.c_uint16 * 25), ("hist", C.c_uint32 * 32), ("ngroups", C.c_uint32)] + \
               [(n, C.c_uint32) for n in ("good", "corrected", "bad", "slips", "acquired", "lost")]


class RdsTrackStats(C.Structure):
    """sdr_rds_track_stats: one channel's bit clock, 32 bytes."""
    _fields_ = [(n, C.c_uint32) for n in ("locked", "phase", "bits", "moves", "half_moves", "resets", "level", "acquired")]


class RdsTrackOpts(C.Structure):
    """sdr_rds_track_opts: the quantisation shift, the bits of acquisition and of the half-bit check."""
    _fields_ = [("qshift", C.c_int), ("acquire_bits", C.c_int), ("half_bits", C.c_int)]


class RdsCarrierStats(C.Structure):
    """sdr_rds_carrier_stats: one channel's carrier phase and smoothed sums, 40 bytes."""
    _fields_ = [("sr", C.c_int64), ("si", C.c_int64), ("st", C.c_int64), ("phi", C.c_int32), ("windows", C.c_uint32),
                ("resets", C.c_uint32), ("reserved", C.c_uint32)]


class RdsCarrierOpts(C.Structure):
    """sdr_rds_carrier_opts: the quantisation shift and the shift of the phasor's smoothing."""
    _fields_ = [("qshift", C.c_int), ("avg_shift", C.c_int)]


class RdsSoftOpts(C.Structure):
    """sdr_rds_soft_opts: sdr_rds_opts and the number of least reliable raw decisions the soft step may flip."""
    _fields_ = [("max_burst", C.c_int), ("loss_blocks", C.c_int), ("soft_bits", C.c_int)]


class RdsSoftStats(C.Structure):
    """sdr_rds_soft_stats: one channel's soft-step counters, 16 bytes."""
    _fields_ = [(n, C.c_uint32) for n in ("soft_blocks", "soft_flips", "soft_bits", "reserved")]


RDS_MAX_GROUPS = 4
RDS_GROUP_SOFT_SHIFT, RDS_SOFT_HISTORY = 4, 32
RDS_TRACK_T, RDS_TRACK_CARRY, RDS_TRACK_MAX_N = 16, 120, 19712
RDS_CARRIER_W, RDS_CARRIER_CORDIC_N = 2048, 24
RDS_GROUP_CPRIME = 0x1
METER_ROW_AUDIO, METER_ROW_RDS = 0x1, 0x2                                   # MeterRow.flags
METER_STEREO, METER_RDS, METER_OFFTUNE, METER_DEAD_AIR = 0x1, 0x2, 0x4, 0x8   # MeterState.flags


def lib() -> C.CDLL:
    """Load libsdr_amd.so (built in-tree by __graft_entry__.build() / `make`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise SdrError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(os.fspath(LIB_PATH))
    vp, sz, i32, f32 = C.c_void_p, C.c_size_t, C.c_int, C.c_float
    sigs = {
        "sdr_last_error": ([], C.c_char_p),
        "sdr_version": ([], i32),
        "sdr_impulse_response_lpf": ([f32, f32, C.c_ushort, vp], i32),
        "sdr_impulse_response_lpf_gain": ([f32, f32, C.c_ushort, i32, vp], i32),
        "sdr_impulse_response_bpf": ([f32, vp, C.c_ushort, vp], i32),
        "sdr_impulse_response_apf": ([f32, C.c_ushort, vp], i32),
        "sdr_impulse_response_rrc": ([f32, C.c_ushort, vp], i32),
        "sdr_convolve_fir": ([vp, sz, vp, sz, i32, i32, vp, i32, vp, i32, i32, vp], i32),
        "sdr_convolve_fir_resample": ([vp, sz, vp, sz, i32, i32, vp, i32, vp, i32, i32, i32, vp], i32),
        "sdr_fm_demod": ([vp, sz, vp, vp, sz, i32, i32, vp, vp], i32),
        "sdr_fm_demod_phase": ([vp, sz, vp, vp, sz, i32, i32, vp, vp], i32),
        "sdr_demod_coeffs": ([vp, i32, C.POINTER(i32)], i32),
        "sdr_meter_deviation": ([i32, C.POINTER(MeterRow)] + [C.POINTER(C.c_double)] * 3, i32),
        "sdr_fmpll": ([vp, sz, vp, sz, i32, i32, f32, f32, vp, f32, f32, f32, vp], i32),
        "sdr_cdr": ([vp, vp, sz, i32, i32, i32, vp], i32),
        "sdr_manchester_decode": ([vp, sz, vp, vp, sz, vp, i32, i32, vp, vp], i32),
        "sdr_differential_decode": ([vp, sz, vp, sz, vp, i32, i32, vp, vp], i32),
        "sdr_ctx_create": ([C.POINTER(vp), i32, i32, i32, i32, i32], i32),
        "sdr_ctx_destroy": ([vp], i32),
        "sdr_ctx_reset": ([vp, vp], i32),
        "sdr_ctx_info": ([vp, C.POINTER(Info)], i32),
        "sdr_frontend": ([vp, vp, sz, vp], i32),
        "sdr_frontend_release_wait": ([vp, vp], i32),
        "sdr_tuner_table": ([i32, vp, i32, C.POINTER(i32)], i32),
        "sdr_tuner_set": ([vp, i32, vp, vp, vp], i32),
        "sdr_tuner_get": ([vp, C.POINTER(i32)], i32),
        "sdr_frontend_tuned": ([vp, vp, sz, vp], i32),
        "sdr_frontend_timing": ([vp, i32], i32),
        "sdr_frontend_times": ([vp, C.POINTER(C.c_double), i32, C.POINTER(i32)], i32),
        "sdr_frontend_stamps": ([vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), i32, C.POINTER(i32)], i32),
        "sdr_mono": ([vp, vp, sz, vp], i32),
        "sdr_stereo": ([vp, vp, sz, vp], i32),
        "sdr_rds_dsp": ([vp, vp, sz, vp], i32),
        "sdr_rds_bits": ([vp, vp, vp, vp, sz, vp, vp, sz, vp], i32),
        "sdr_get_fm_demod": ([vp, vp, sz, vp], i32),
        "sdr_push_fm_demod": ([vp, vp, sz, vp], i32),
        "sdr_stereo_pre": ([vp, vp], i32),
        "sdr_stereo_pll": ([vp, vp], i32),
        "sdr_stereo_post": ([vp, vp, sz, vp], i32),
        "sdr_rds_pre": ([vp, vp], i32),
        "sdr_pre": ([vp, vp], i32),
        "sdr_rds_pll": ([vp, vp], i32),
        "sdr_plls": ([vp, vp], i32),
        "sdr_plls_launch": ([vp, i32, vp], i32),
        "sdr_plls_prepare": ([vp, i32, vp], i32),
        "sdr_plls_fits": ([vp, i32, i32, i32, C.POINTER(i32), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)], i32),
        "sdr_diag_plls_plan": ([vp, i32, i32, i32, C.POINTER(i32)], i32),
        "sdr_plls_launch_sel": ([vp, i32, i32, vp], i32),
        "sdr_plls_signal": ([vp, vp], i32),
        "sdr_frontend_pre_parts": ([vp, vp, sz, i32, vp], i32),
        "sdr_plls_wait": ([vp, vp], i32),
        "sdr_plls_report": ([vp, C.POINTER(C.c_double), i32, C.POINTER(i32), vp], i32),
        "sdr_plls_cycles": ([vp, C.POINTER(C.c_double), C.POINTER(C.c_double), vp], i32),
        "sdr_plls_block_cycles": ([vp, C.POINTER(C.c_double), C.POINTER(C.c_double), i32, C.POINTER(C.c_int), vp], i32),
        "sdr_plls_timeline": ([vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), i32, C.POINTER(i32), vp], i32),
        "sdr_rds_post": ([vp, vp, sz, vp], i32),
        "sdr_ctx_buffer": ([vp, C.c_char_p, C.POINTER(vp), C.POINTER(sz), C.POINTER(i32)], i32),
        "sdr_ctx_rds_clean_q": ([vp, C.POINTER(vp), C.POINTER(sz), C.POINTER(i32)], i32),
        "sdr_hbm_copy": ([vp, vp, sz, vp], i32),
        "sdr_scan_geometry": ([i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)], i32),
        "sdr_scan_window": ([i32, vp, i32, C.POINTER(i32)], i32),
        "sdr_scan_opts_default": ([C.POINTER(ScanOpts)], None),
        "sdr_scan_pick": ([i32, vp, C.POINTER(ScanOpts), vp, vp, i32, C.POINTER(i32)], i32),
        "sdr_scan_create": ([C.POINTER(vp), i32, i32, i32], i32),
        "sdr_scan_destroy": ([vp], i32),
        "sdr_scan_reset": ([vp, vp], i32),
        "sdr_scan_block": ([vp, vp, sz, vp], i32),
        "sdr_scan_psd": ([vp, vp, C.POINTER(C.c_longlong), vp], i32),
        "sdr_split_geometry": ([i32, i32] + [C.POINTER(i32)] * 5, i32),
        "sdr_split_taps": ([i32, vp, i32, C.POINTER(i32)], i32),
        "sdr_split_create": ([C.POINTER(vp), i32, i32, i32, i32, i32], i32),
        "sdr_split_destroy": ([vp], i32),
        "sdr_split_reset": ([vp, vp], i32),
        "sdr_split_block": ([vp, vp, sz, vp, sz, vp], i32),
        "sdr_split_clips": ([vp, vp, vp], i32),
        "sdr_split16_create": ([C.POINTER(vp), i32, i32, i32, i32, i32], i32),
        "sdr_split16_check": ([i32, i32, i32, i32], i32),
        "sdr_split16_destroy": ([vp], i32),
        "sdr_split16_reset": ([vp, vp], i32),
        "sdr_split16_set_shifts": ([vp, vp, vp], i32),
        "sdr_split16_block": ([vp, vp, sz, vp, sz, vp], i32),
        "sdr_split16_clips": ([vp, vp, vp], i32),
        "sdr_split16_peaks": ([vp, vp, i32, vp], i32),
        "sdr_split16_shift_for": ([C.c_longlong, i32, i32], i32),
        "sdr_meter_taps": ([i32, vp, i32, C.POINTER(i32)], i32),
        "sdr_meter_opts_default": ([C.POINTER(MeterOpts)], None),
        "sdr_meter_status": ([i32, C.POINTER(MeterRow), C.POINTER(MeterOpts), C.POINTER(MeterState)], i32),
        "sdr_meter_create": ([C.POINTER(vp), i32, i32, i32], i32),
        "sdr_meter_destroy": ([vp], i32),
        "sdr_meter_reset": ([vp, vp], i32),
        "sdr_meter_audio": ([vp, vp, vp, sz, vp], i32),
        "sdr_meter_rds": ([vp, vp, vp], i32),
        "sdr_meter_read": ([vp, vp, vp], i32),
        "sdr_meter_rows": ([vp, C.POINTER(vp)], i32),
        "sdr_meter_rf": ([vp, vp, vp], i32),
        "sdr_meter_rf_read": ([vp, vp, vp], i32),
        "sdr_meter_rf_rows": ([vp, C.POINTER(vp)], i32),
        "sdr_meter_rf_opts_default": ([C.POINTER(MeterRfOpts)], None),
        "sdr_meter_rf_status": ([i32, C.POINTER(MeterRfRow), C.POINTER(MeterRfOpts), C.POINTER(MeterRfState)], i32),
        "sdr_audio_opts_default": ([C.POINTER(AudioOpts)], None),
        "sdr_audio_coeffs": ([i32, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)], i32),
        "sdr_audio_create": ([C.POINTER(vp), i32, i32, i32, i32, C.POINTER(AudioOpts)], i32),
        "sdr_audio_destroy": ([vp], i32),
        "sdr_audio_reset": ([vp, vp], i32),
        "sdr_audio_set_control": ([vp, vp, vp, vp], i32),
        "sdr_audio_blend_from_meter": ([vp, vp, vp], i32),
        "sdr_audio_finish": ([vp, vp, sz, vp, sz, vp], i32),
        "sdr_audio_read_state": ([vp, vp, vp], i32),
        "sdr_rds_opts_default": ([C.POINTER(RdsOpts)], None),
        "sdr_rds_syndrome": ([C.c_uint32], C.c_uint32),
        "sdr_rds_correction_table": ([i32, vp, C.POINTER(i32)], i32),
        "sdr_rds_mode_ok": ([i32], i32),
        "sdr_rds_dec_create": ([C.POINTER(vp), i32, i32, C.POINTER(RdsOpts)], i32),
        "sdr_rds_dec_destroy": ([vp], i32),
        "sdr_rds_dec_reset": ([vp, vp], i32),
        "sdr_rds_groups": ([vp, vp, vp, sz, vp], i32),
        "sdr_rds_groups_read": ([vp, vp, vp, vp], i32),
        "sdr_rds_groups_copy": ([vp, vp, vp, vp], i32),
        "sdr_rds_stats_read": ([vp, vp, vp], i32),
        "sdr_rds_soft_opts_default": ([C.POINTER(RdsSoftOpts)], None),
        "sdr_rds_dec_create_soft": ([C.POINTER(vp), i32, i32, C.POINTER(RdsSoftOpts)], i32),
        "sdr_rds_groups_soft": ([vp, vp, vp, sz, vp, sz, vp], i32),
        "sdr_rds_soft_stats_read": ([vp, vp, vp], i32),
        "sdr_rds_track_bits_soft": ([vp, vp, sz, i32, vp, vp, sz, vp, sz, vp], i32),
        "sdr_rds_track_opts_default": ([C.POINTER(RdsTrackOpts)], None),
        "sdr_rds_track_create": ([C.POINTER(vp), i32, i32, i32, C.POINTER(RdsTrackOpts)], i32),
        "sdr_rds_track_destroy": ([vp], i32),
        "sdr_rds_track_reset": ([vp, vp], i32),
        "sdr_rds_track_bits": ([vp, vp, sz, i32, vp, vp, sz, vp], i32),
        "sdr_rds_track_stats_read": ([vp, vp, vp], i32),
        "sdr_rds_carrier_opts_default": ([C.POINTER(RdsCarrierOpts)], None),
        "sdr_rds_carrier_create": ([C.POINTER(vp), i32, i32, i32, C.POINTER(RdsCarrierOpts)], i32),
        "sdr_rds_carrier_destroy": ([vp], i32),
        "sdr_rds_carrier_reset": ([vp, vp], i32),
        "sdr_rds_carrier_rotate": ([vp, vp, sz, vp, sz, i32, vp, sz, vp], i32),
        "sdr_rds_carrier_stats_read": ([vp, vp, vp], i32),
        "sdr_rds_station_init": ([C.POINTER(RdsStationC)], None),
        "sdr_rds_station_update": ([C.POINTER(RdsStationC), C.POINTER(RdsGroup)], None),
        "sdr_rds_station_stats": ([C.POINTER(RdsStationC), C.POINTER(RdsStats)], None),
        "sdr_rds_station_bler": ([C.POINTER(RdsStationC)], C.c_double),
        "sdr_rds_pty_name": ([i32], C.c_char_p),
        "sdr_rds_station_format": ([C.POINTER(RdsStationC), C.c_char_p, sz], sz),
    }
    for name, (args, res) in sigs.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def check(rc: int, what: str = "") -> None:
    if rc != SDR_OK:
        msg = lib().sdr_last_error().decode(errors="replace")
        raise SdrError(f"{what} failed ({rc}): {msg}", rc)


def hbm_copy(dst, src, stream=None) -> None:
    """dst <- src (same byte size, 16-byte aligned device tensors) with the calibration copy kernel
    (sdr_hbm_copy): the HBM rate a plain stream reaches, for the benchmark's roofline context."""
    nbytes = src.numel() * src.element_size()
    if dst.numel() * dst.element_size() != nbytes:
        raise SdrError("hbm_copy: size mismatch")
    check(lib().sdr_hbm_copy(_ptr(dst), _ptr(src), nbytes, _stream(stream)), "sdr_hbm_copy")


# ------------------------------------------------------------------ torch plumbing helpers
def _ptr(t) -> int | None:
    if t is None:
        return None
    return int(t.data_ptr())


def _stream(stream=None) -> int | None:
    if stream is not None:
        return int(stream.cuda_stream) if hasattr(stream, "cuda_stream") else int(stream)
    import torch
    return int(torch.cuda.current_stream().cuda_stream) or None


def _opts(struct, default_fn_name: str, label: str, **opts):
    """An options record: the library's defaults (default_fn_name) with the given fields replaced."""
    o = struct()
    getattr(lib(), default_fn_name)(C.byref(o))
    for k, v in opts.items():
        if k not in dict(struct._fields_):
            raise SdrError(f"{label}: unknown option {k}", -1)
        setattr(o, k, v)
    return o


def _dtype(struct):
    """numpy dtype of a record of the C ABI."""
    import numpy as np
    return np.dtype(struct)


class _Handle:
    """What the stage handles share: ._h (made by the subclass) is destroyed once, by close() or at the
    object's end; reset(); and the read of one record per channel. _destroy and _reset name the library's calls."""
    _destroy = _reset = ""

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, stream=None):
        check(getattr(lib(), self._reset)(self._h, _stream(stream)), self._reset)

    def _records(self, fn_name: str, dtype, stream=None):
        """numpy structured array [nch] filled by fn_name(handle, host, stream); synchronises the stream."""
        import numpy as np
        out = np.zeros(self.nch, dtype)
        check(getattr(lib(), fn_name)(self._h, out.ctypes.data_as(C.c_void_p), _stream(stream)), fn_name)
        return out


def _row_stride(t) -> int:
    """Elements between consecutive channels of a 2-D [nch][len] tensor (last dim contiguous)."""
    assert t.dim() == 2 and t.stride(1) == 1, "expected a [nch][len] tensor with a contiguous last dim"
    return int(t.stride(0))


# ------------------------------------------------------------------ tap design (host)
def _taps(fn, n, *args):
    import numpy as np
    h = np.zeros(n, np.float32)
    check(fn(*args, h.ctypes.data_as(C.c_void_p)), fn.__name__)
    return h


def impulse_response_lpf(Fs, Fc, num_taps, u=None):
    """impulseResponseLPF, src/filter.cpp:13-29 (u=None) or :33-50 (integer gain u)."""
    if u is None:
        return _taps(lib().sdr_impulse_response_lpf, num_taps, Fs, Fc, num_taps)
    return _taps(lib().sdr_impulse_response_lpf_gain, num_taps, Fs, Fc, num_taps, u)


def impulse_response_bpf(Fs, f0, f1, num_taps):
    """impulseResponseBPF, src/filter.cpp:55-71."""
    import numpy as np
    fb = np.array([f0, f1], np.float32)
    return _taps(lib().sdr_impulse_response_bpf, num_taps, Fs, fb.ctypes.data_as(C.c_void_p), num_taps)


def impulse_response_apf(gain, num_taps):
    """impulseResponseAPF, src/filter.cpp:73-78."""
    return _taps(lib().sdr_impulse_response_apf, num_taps, gain, num_taps)


def impulse_response_rrc(Fs, num_taps):
    """impulseResponseRRC, src/filter.cpp:80-102."""
    return _taps(lib().sdr_impulse_response_rrc, num_taps, Fs, num_taps)


def tuner_table(mode: int):
    """The shared-capture tuner's rotator table of a mode (host only): [N, 2] f32 (cos, sin)(2 pi i / N),
    N = rf_Fs / 1000, each the real value correctly rounded (sdr_tuner_table)."""
    import numpy as np
    n = C.c_int(0)
    if lib().sdr_tuner_table(mode, None, 0, C.byref(n)) != SDR_OK:
        raise SdrError(f"sdr_tuner_table: mode {mode} not in 0..3", -1)
    t = np.zeros((n.value, 2), np.float32)
    if lib().sdr_tuner_table(mode, t.ctypes.data_as(C.c_void_p), n.value, C.byref(n)) != SDR_OK:
        raise SdrError("sdr_tuner_table failed", -1)
    return t


# ------------------------------------------------------------------ band scan (include/sdr_amd.h, sdr_scan_*)
def scan_geometry(mode: int) -> tuple[int, int, int]:
    """(N bins = rf_Fs / 1000, segments per block, block_iq) of a mode (host only)."""
    n, s, b = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib().sdr_scan_geometry(mode, C.byref(n), C.byref(s), C.byref(b)), "sdr_scan_geometry")
    return n.value, s.value, b.value


def scan_window(mode: int):
    """The scan's f32 Hann table [N]: RN32(0.5 - 0.5 cos(2 pi j / N)) (host only)."""
    import numpy as np
    w = np.zeros(scan_geometry(mode)[0], np.float32)
    n = C.c_int(0)
    check(lib().sdr_scan_window(mode, w.ctypes.data_as(C.c_void_p), w.size, C.byref(n)), "sdr_scan_window")
    return w


def scan_opts(**opts) -> ScanOpts:
    """The picker's defaults (sdr_scan_opts_default) with the given fields replaced."""
    return _opts(ScanOpts, "sdr_scan_opts_default", "scan_pick", **opts)


def scan_pick(mode: int, psd_row, max=None, **opts):
    """The stations of one spectrum row [N] (sdr_scan_pick; host only): (khz int32, db f32) in
    descending channel power. opts: half_width_khz, step_khz, first_khz, sep_khz, guard_khz, thr_db.
    max: write at most this many (the arrays then hold min(max, found) entries)."""
    import numpy as np
    N = scan_geometry(mode)[0]
    row = np.ascontiguousarray(psd_row, np.float32)
    if row.shape != (N,):
        raise SdrError(f"scan_pick: psd_row must have {N} entries", -1)
    o = scan_opts(**opts)
    cap = N + 1 if max is None else int(max)
    khz, db = np.zeros(cap, np.int32), np.zeros(cap, np.float32)
    n = C.c_int(0)
    check(lib().sdr_scan_pick(mode, row.ctypes.data_as(C.c_void_p), C.byref(o), khz.ctypes.data_as(C.c_void_p),
                              db.ctypes.data_as(C.c_void_p), cap, C.byref(n)), "sdr_scan_pick")
    k = min(n.value, cap)
    return khz[:k], db[:k]


class Scanner(_Handle):
    """The band scan of `nsrc` capture rows of one mode (sdr_scan_*): block(iq) per block of the rows
    sdr_frontend_tuned reads, then psd() or stations(). Its own handle: no channels, any stream."""

    _destroy, _reset = "sdr_scan_destroy", "sdr_scan_reset"

    def __init__(self, mode: int, nsrc: int, device: int = 0):
        h = C.c_void_p()
        check(lib().sdr_scan_create(C.byref(h), device, mode, nsrc), "sdr_scan_create")
        self._h = h
        self.mode, self.nsrc, self.device = mode, nsrc, device
        self.n_bins, self.segments_per_block, self.block_iq = scan_geometry(mode)

    def block(self, iq, stream=None):
        """iq: uint8 [nsrc][2*block_iq] (device); enqueues, no sync."""
        if iq.dim() != 2 or iq.shape[0] != self.nsrc:
            raise SdrError(f"Scanner.block: expected [{self.nsrc}][2*block_iq] rows", -1)
        stride = _row_stride(iq) if iq.shape[0] > 1 else int(iq.shape[1])
        check(lib().sdr_scan_block(self._h, _ptr(iq), stride, _stream(stream)), "sdr_scan_block")

    def psd(self, stream=None):
        """(numpy f32 [nsrc][N], segments accumulated per row); synchronises the stream."""
        import numpy as np
        out = np.zeros((self.nsrc, self.n_bins), np.float32)
        seg = C.c_longlong(0)
        check(lib().sdr_scan_psd(self._h, out.ctypes.data_as(C.c_void_p), C.byref(seg), _stream(stream)),
              "sdr_scan_psd")
        return out, seg.value

    def stations(self, stream=None, **opts):
        """(src, khz) int32 arrays over all rows, row after row, each row in the picker's order:
        ready for Pipeline.set_tuning."""
        import numpy as np
        psd, _ = self.psd(stream)
        src, khz = [], []
        for r in range(self.nsrc):
            k, _db = scan_pick(self.mode, psd[r], **opts)
            src.append(np.full(k.size, r, np.int32))
            khz.append(k)
        return np.concatenate(src), np.concatenate(khz)


# ------------------------------------------------------------------ wideband splitter (include/sdr_amd.h, sdr_split_*)
def split_geometry(mode: int, W: int) -> tuple[int, int, int, int, int]:
    """(rows R = 2 W - 1, taps T = 16 W, wide_iq = W * block_iq, half_khz = N / 2, default shift) of a
    mode and a width factor W in {4, 8, 10} (host only)."""
    v = [C.c_int(0) for _ in range(5)]
    check(lib().sdr_split_geometry(mode, W, *[C.byref(x) for x in v]), "sdr_split_geometry")
    return tuple(x.value for x in v)


def split_taps(W: int):
    """The splitter's tap table: int16 [R][T][2] (g_re, g_im) (host only)."""
    import numpy as np
    n = C.c_int(0)
    check(lib().sdr_split_taps(W, None, 0, C.byref(n)), "sdr_split_taps")
    g = np.zeros((2 * W - 1, 16 * W, 2), np.int16)
    check(lib().sdr_split_taps(W, g.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), "sdr_split_taps")
    return g


class Splitter(_Handle):
    """`nwide` wide int8 I/Q captures at W * rf_Fs into nwide * (2 W - 1) capture rows at rf_Fs, the rows
    sdr_frontend_tuned and the Scanner read (sdr_split_*). Its own handle: no channels, any stream."""

    _c, _name, _dtype, _bytes = "sdr_split", "Splitter", "int8", 1    # the C prefix; of a value: torch dtype, bytes
    _destroy = property(lambda self: self._c + "_destroy")
    _reset = property(lambda self: self._c + "_reset")

    def __init__(self, W: int, nwide: int, mode: int = 0, device: int = 0, shift=None):
        h = C.c_void_p()
        create = getattr(lib(), self._c + "_create")
        check(create(C.byref(h), device, mode, W, nwide, 0 if shift is None else int(shift)), self._c + "_create")
        self._h = h
        self.W, self.nwide, self.mode, self.device = W, nwide, mode, device
        self.rows, self.taps, self.wide_iq, self.half_khz, d = split_geometry(mode, W)
        self.block_iq = self.wide_iq // W
        self._set_shift(d, None if shift is None or shift <= 0 else int(shift))

    def _set_shift(self, d: int, shift):
        """d: split_geometry's default shift; shift: the constructor's, or None for the default."""
        self.shift = d if shift is None else shift

    def block(self, wide, out=None, stream=None):
        """wide: int8 (Splitter16: int16) [nwide][2*W*block_iq] (device). Returns the uint8 rows
        [nwide*R][2*block_iq] (out, or a new tensor); enqueues, no sync."""
        import torch
        if wide.dim() != 2 or wide.shape[0] != self.nwide or wide.dtype != getattr(torch, self._dtype):
            raise SdrError(f"{self._name}.block: expected {self._dtype} [{self.nwide}][2*W*block_iq] streams", -1)
        if out is None:
            out = torch.empty((self.nwide * self.rows, 2 * self.block_iq), dtype=torch.uint8, device=wide.device)
        elif out.dim() != 2 or out.shape[0] != self.nwide * self.rows or out.dtype != torch.uint8:
            raise SdrError(f"{self._name}.block: expected uint8 [{self.nwide * self.rows}][2*block_iq] rows", -1)
        ws = _row_stride(wide) if wide.shape[0] > 1 else int(wide.shape[1])
        check(getattr(lib(), self._c + "_block")(self._h, _ptr(wide), self._bytes * ws, _ptr(out), _row_stride(out),
                                                 _stream(stream)), self._c + "_block")
        return out

    def _read(self, what, *args, stream=None):
        """numpy int64 [nwide][R] of sdr_split*_<what>; synchronises the stream."""
        import numpy as np
        c = np.zeros((self.nwide, self.rows), np.int64)
        check(getattr(lib(), f"{self._c}_{what}")(self._h, c.ctypes.data_as(C.c_void_p), *args, _stream(stream)),
              f"{self._c}_{what}")
        return c

    def clips(self, stream=None):
        """numpy int64 [nwide][R]: clipped output components since the last reset; synchronises the stream."""
        return self._read("clips", stream=stream)


def split16_shift_for(peak: int, target: int = 90, *, W: int) -> int:
    """The 16-bit splitter's gain rule (host only): the smallest shift in 1..33 at which `peak` rounds to at most
    `target` (1..127); W's default shift for a peak of 0."""
    s = lib().sdr_split16_shift_for(int(peak), int(target), int(W))
    if s < 1:
        check(s, "sdr_split16_shift_for")
    return s


class Splitter16(Splitter):
    """The Splitter for wide int16 I/Q captures (sdr_split16_*): a shift per stream and row (set_shifts) and a
    peak reading per row (peaks), so that each row can have its own gain. Its own handle: any stream."""

    _c, _name, _dtype, _bytes = "sdr_split16", "Splitter16", "int16", 2

    def _set_shift(self, d: int, shift):
        import numpy as np
        self.shift_default = d + 8
        self._shifts = np.full((self.nwide, self.rows), self.shift_default if shift is None else shift, np.int32)

    @property
    def shifts(self):
        """numpy int32 [nwide][R]: the table of the last set_shifts (or the shift of the constructor); a copy."""
        return self._shifts.copy()

    def set_shifts(self, shifts, stream=None):
        """shifts: ints [nwide][R] (or nwide * R), each in 1..33. Holds for the block calls enqueued after it on
        the stream; no sync. A refused table changes nothing."""
        import numpy as np
        t = np.ascontiguousarray(np.asarray(shifts), np.int32)
        if t.size != self.nwide * self.rows:
            raise SdrError(f"Splitter16.set_shifts: expected {self.nwide} x {self.rows} shifts", -1)
        check(lib().sdr_split16_set_shifts(self._h, t.ctypes.data_as(C.c_void_p), _stream(stream)),
              "sdr_split16_set_shifts")
        self._shifts = t.reshape(self.nwide, self.rows).copy()

    def peaks(self, clear: bool = False, stream=None):
        """numpy int64 [nwide][R]: the largest |acc_re| or |acc_im| of each row since the last reset or clearing
        read (clear=True makes this one); independent of the shifts; synchronises the stream."""
        return self._read("peaks", 1 if clear else 0, stream=stream)


# ------------------------------------------------------------------ reception meter (include/sdr_amd.h, sdr_meter_*)
def meter_row_dtype():
    """numpy dtype of sdr_meter_row (64 bytes)."""
    return _dtype(MeterRow)


def meter_taps(mode: int):
    """The meter's noise band-pass [101]: impulse_response_bpf(if_Fs, 75e3, 84e3, 101) (host only)."""
    import numpy as np
    n = C.c_int(0)
    check(lib().sdr_meter_taps(mode, None, 0, C.byref(n)), "sdr_meter_taps")
    h = np.zeros(n.value, np.float32)
    check(lib().sdr_meter_taps(mode, h.ctypes.data_as(C.c_void_p), h.size, C.byref(n)), "sdr_meter_taps")
    return h


def meter_opts(**opts) -> MeterOpts:
    """The status thresholds' defaults (sdr_meter_opts_default) with the given fields replaced."""
    return _opts(MeterOpts, "sdr_meter_opts_default", "meter_status", **opts)


def meter_status(mode: int, rows, **opts):
    """sdr_meter_status of every row (host only): rows is a MeterRow or a numpy array of
    meter_row_dtype(); returns a numpy structured array (offset, level_db, pilot_nr, rds_nr, eye_db,
    flags) of the same shape. The readings are discriminator units and ratios, not kHz of deviation.
    opts: pilot_nr_min, rds_nr_min, offtune_min, silence_peak."""
    import numpy as np
    o = meter_opts(**opts)
    if isinstance(rows, MeterRow):
        rows = np.frombuffer(bytes(rows), dtype=meter_row_dtype())[0]
    rows = np.asarray(rows, dtype=meter_row_dtype())
    flat = np.ascontiguousarray(rows).reshape(-1)
    out = np.zeros(flat.shape, np.dtype(MeterState))
    st = MeterState()
    for i in range(flat.size):
        row = MeterRow.from_buffer_copy(flat[i].tobytes())
        check(lib().sdr_meter_status(mode, C.byref(row), C.byref(o), C.byref(st)), "sdr_meter_status")
        out[i] = (st.offset, st.level_db, st.pilot_nr, st.rds_nr, st.eye_db, st.flags)
    return out.reshape(rows.shape)


def meter_deviation(mode: int, rows):
    """sdr_meter_deviation of every row (host only): a numpy structured array (peak_khz, rms_khz,
    offset_khz) of the rows' shape. Deviation in kHz only for rows of a PHASE_DEMOD pipeline."""
    import numpy as np
    if isinstance(rows, MeterRow):
        rows = np.frombuffer(bytes(rows), dtype=meter_row_dtype())[0]
    rows = np.asarray(rows, dtype=meter_row_dtype())
    flat = np.ascontiguousarray(rows).reshape(-1)
    out = np.zeros(flat.shape, np.dtype([("peak_khz", "f8"), ("rms_khz", "f8"), ("offset_khz", "f8")]))
    pk, rms, off = C.c_double(), C.c_double(), C.c_double()
    for i in range(flat.size):
        row = MeterRow.from_buffer_copy(flat[i].tobytes())
        check(lib().sdr_meter_deviation(mode, C.byref(row), C.byref(pk), C.byref(rms), C.byref(off)),
              "sdr_meter_deviation")
        out[i] = (pk.value, rms.value, off.value)
    return out.reshape(rows.shape)


def meter_rf_row_dtype():
    """numpy dtype of sdr_meter_rf_row (32 bytes)."""
    return _dtype(MeterRfRow)


def meter_rf_opts(**opts) -> MeterRfOpts:
    """The RF status threshold's default (sdr_meter_rf_opts_default) with the given fields replaced."""
    return _opts(MeterRfOpts, "sdr_meter_rf_opts_default", "meter_rf_status", **opts)


def meter_rf_status(mode: int, rows, **opts):
    """sdr_meter_rf_status of every row (host only): rows is a MeterRfRow or a numpy array of
    meter_rf_row_dtype() -- a block's, or a run-long one summed as include/sdr_amd.h says; returns a numpy
    structured array (level_dbfs, ripple, cnr_db, fade_db, crest_db, flags) of the same shape.
    opts: ripple_max."""
    import numpy as np
    o = meter_rf_opts(**opts)
    if isinstance(rows, MeterRfRow):
        rows = np.frombuffer(bytes(rows), dtype=meter_rf_row_dtype())[0]
    rows = np.asarray(rows, dtype=meter_rf_row_dtype())
    flat = np.ascontiguousarray(rows).reshape(-1)
    out = np.zeros(flat.shape, np.dtype(MeterRfState))
    st = MeterRfState()
    for i in range(flat.size):
        row = MeterRfRow.from_buffer_copy(flat[i].tobytes())
        check(lib().sdr_meter_rf_status(mode, C.byref(row), C.byref(o), C.byref(st)), "sdr_meter_rf_status")
        out[i] = (st.level_dbfs, st.ripple, st.cnr_db, st.fade_db, st.crest_db, st.flags)
    return out.reshape(rows.shape)


class Meter(_Handle):
    """The reception meter of `nch` channels of one mode (sdr_meter_*): per block audio(pipe, lr) after
    the block's stereo stage and rds(pipe) after its RDS stage -- on one Pipeline or on two joined by
    push_fm_demod -- then rows() or status(). Its own handle; the rows stay on the device."""

    _destroy, _reset = "sdr_meter_destroy", "sdr_meter_reset"

    def __init__(self, nch: int, mode: int = 0, device: int = 0):
        h = C.c_void_p()
        check(lib().sdr_meter_create(C.byref(h), device, nch, mode), "sdr_meter_create")
        self._h = h
        self.nch, self.mode, self.device = nch, mode, device

    def audio(self, pipe: "Pipeline", lr=None, stream=None):
        """The fm, pilot, noise and audio fields of pipe's current block; lr: the int16 [nch][2*n_audio]
        tensor stereo() / stereo_post() wrote (None: the audio fields stay 0). Enqueues, no sync."""
        stride = 0 if lr is None else (_row_stride(lr) if lr.shape[0] > 1 else int(lr.shape[1]))
        check(lib().sdr_meter_audio(self._h, pipe._h, _ptr(lr), stride, _stream(stream)), "sdr_meter_audio")

    def rds(self, pipe: "Pipeline", stream=None):
        """rds_sq and the eye fields of pipe's current block (after rds() / rds_post())."""
        check(lib().sdr_meter_rds(self._h, pipe._h, _stream(stream)), "sdr_meter_rds")

    def rf(self, pipe: "Pipeline", stream=None):
        """The IF envelope readings of pipe's current block (an IF_ENVELOPE pipeline, after its front end), into
        rows of their own. Enqueues, no sync."""
        check(lib().sdr_meter_rf(self._h, pipe._h, _stream(stream)), "sdr_meter_rf")

    def read_rf(self, stream=None):
        """numpy structured array [nch] of meter_rf_row_dtype(); synchronises the stream."""
        return self._records("sdr_meter_rf_read", meter_rf_row_dtype(), stream)

    def rf_rows(self) -> int:
        """Device address of the RF rows [nch] (sdr_meter_rf_rows)."""
        p = C.c_void_p()
        check(lib().sdr_meter_rf_rows(self._h, C.byref(p)), "sdr_meter_rf_rows")
        return int(p.value)

    def rf_rows_into(self, out, stream=None):
        """The RF rows copied on the device into `out` (a contiguous uint8 tensor of nch * 32 bytes) in `stream`'s
        order, without synchronising (as rows_into)."""
        nbytes = self.nch * C.sizeof(MeterRfRow)
        if out.numel() * out.element_size() != nbytes or not out.is_contiguous():
            raise SdrError(f"Meter.rf_rows_into: expected a contiguous tensor of {nbytes} bytes", -1)
        rc = _hip().hipMemcpyAsync(C.c_void_p(out.data_ptr()), C.c_void_p(self.rf_rows()), C.c_size_t(nbytes),
                                   C.c_int(3), C.c_void_p(_stream(stream)))
        if rc != 0:
            raise SdrError(f"hipMemcpyAsync failed ({rc})")
        return out

    def rows(self, stream=None):
        """numpy structured array [nch] of meter_row_dtype(); synchronises the stream."""
        return self._records("sdr_meter_read", meter_row_dtype(), stream)

    def rows_into(self, out, stream=None):
        """The rows copied on the device into `out` (a contiguous uint8 tensor of nch * 64 bytes) in
        `stream`'s order, without synchronising: for schedules that keep every block's rows."""
        nbytes = self.nch * C.sizeof(MeterRow)
        if out.numel() * out.element_size() != nbytes or not out.is_contiguous():
            raise SdrError(f"Meter.rows_into: expected a contiguous tensor of {nbytes} bytes", -1)
        rc = _hip().hipMemcpyAsync(C.c_void_p(out.data_ptr()), C.c_void_p(self.rows_ptr()), C.c_size_t(nbytes),
                                   C.c_int(3), C.c_void_p(_stream(stream)))
        if rc != 0:
            raise SdrError(f"hipMemcpyAsync failed ({rc})")
        return out

    def rows_ptr(self) -> int:
        """Device address of the rows [nch] (sdr_meter_rows)."""
        p = C.c_void_p()
        check(lib().sdr_meter_rows(self._h, C.byref(p)), "sdr_meter_rows")
        return int(p.value)

    def status(self, stream=None, **opts):
        """meter_status of the current rows (synchronises the stream)."""
        return meter_status(self.mode, self.rows(stream), **opts)


# ------------------------------------------------------------------ audio finishing (include/sdr_amd.h, sdr_audio_*)
def audio_coeffs(mode: int, tau_us: float):
    """(a, b) of the de-emphasis one-pole y = a y + b x at the mode's audio rate, as numpy float32
    (host only): a = RN32(exp(-1e6 / (tau_us Fs_a))), b = RN32(1 - a); tau_us = 0 gives (0, 1)."""
    import numpy as np
    a, b = C.c_float(), C.c_float()
    check(lib().sdr_audio_coeffs(mode, tau_us, C.byref(a), C.byref(b)), "sdr_audio_coeffs")
    return np.float32(a.value), np.float32(b.value)


def audio_opts(**opts) -> AudioOpts:
    """The finishing stage's defaults (sdr_audio_opts_default) with the given fields replaced."""
    return _opts(AudioOpts, "sdr_audio_opts_default", "audio_opts", **opts)


def audio_state_dtype():
    """numpy dtype of sdr_audio_state (24 bytes)."""
    return _dtype(AudioState)


class AudioFinish(_Handle):
    """The finishing stage of `nch` channels of one mode (sdr_audio_*): de-emphasis, stereo blend and
    gain over the int16 rows stereo() (width 2) or mono() (width 1) wrote. Per block, optionally
    set_control(blend, gain) or blend_from_meter(meter) after meter.audio, then finish(lr). Its own handle;
    the state stays on the device. opts: tau_us (75; 50 outside the Americas; 0 off), blend_lo, blend_hi."""

    _destroy, _reset = "sdr_audio_destroy", "sdr_audio_reset"

    def __init__(self, nch: int, mode: int = 0, width: int = 2, device: int = 0, **opts):
        h = C.c_void_p()
        o = audio_opts(**opts)
        check(lib().sdr_audio_create(C.byref(h), device, nch, mode, width, C.byref(o)), "sdr_audio_create")
        self._h = h
        self.nch, self.mode, self.width, self.device = nch, mode, width, device

    def set_control(self, blend=None, gain=None, stream=None):
        """New targets per channel (a scalar serves every channel): blend in [0, 1] (0 mono, 1 full
        stereo), gain >= 0 (0 mutes); each is reached by a linear ramp over the next block."""
        import numpy as np
        arr = [None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (self.nch,)))
               for v in (blend, gain)]
        ptr = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in arr]
        check(lib().sdr_audio_set_control(self._h, ptr[0], ptr[1], _stream(stream)), "sdr_audio_set_control")

    def blend_from_meter(self, meter: "Meter", stream=None):
        """The blend targets from the meter's current rows (after meter.audio of the block, same stream)."""
        check(lib().sdr_audio_blend_from_meter(self._h, meter._h, _stream(stream)), "sdr_audio_blend_from_meter")

    def finish(self, lr, out=None, stream=None):
        """One block: lr int16 [nch][>= width * n_audio] to out (a new tensor when None; out may be lr)."""
        import torch
        if out is None:
            out = torch.empty(self.nch, lr.shape[1], dtype=torch.int16, device=lr.device)
        check(lib().sdr_audio_finish(self._h, _ptr(lr), _row_stride(lr), _ptr(out), _row_stride(out), _stream(stream)),
              "sdr_audio_finish")
        return out

    def state(self, stream=None):
        """numpy structured array [nch] of audio_state_dtype(); synchronises the stream."""
        return self._records("sdr_audio_read_state", audio_state_dtype(), stream)


# ------------------------------------------------------------------ RDS group decoder (include/sdr_amd.h, sdr_rds_*)
def rds_group_dtype():
    """numpy dtype of sdr_rds_group (16 bytes)."""
    return _dtype(RdsGroup)


def rds_stats_dtype():
    """numpy dtype of sdr_rds_stats (32 bytes)."""
    return _dtype(RdsStats)


def rds_syndrome(w26: int) -> int:
    """The 10-bit syndrome of a 26-bit RDS block (host only)."""
    return int(lib().sdr_rds_syndrome(int(w26) & 0xFFFFFFFF))


def rds_correction_table(max_burst: int = 2):
    """(tab, entries): tab[syndrome] = the burst error pattern it corrects, 0 elsewhere (host only)."""
    import numpy as np
    tab = np.zeros(1024, np.uint32)
    n = C.c_int(0)
    check(lib().sdr_rds_correction_table(max_burst, tab.ctypes.data_as(C.c_void_p), C.byref(n)),
          "sdr_rds_correction_table")
    return tab, n.value


def rds_opts(**opts) -> RdsOpts:
    """The decoder's defaults (sdr_rds_opts_default) with the given fields replaced."""
    return _opts(RdsOpts, "sdr_rds_opts_default", "rds_opts", **opts)


def rds_soft_opts(**opts) -> RdsSoftOpts:
    """The soft decoder's defaults (sdr_rds_soft_opts_default) with the given fields replaced."""
    return _opts(RdsSoftOpts, "sdr_rds_soft_opts_default", "rds_soft_opts", **opts)


def rds_soft_stats_dtype():
    """numpy dtype of sdr_rds_soft_stats (16 bytes)."""
    return _dtype(RdsSoftStats)


class RdsDecoder(_Handle):
    """The RDS group decoder of `nch` channels (sdr_rds_*): block sync with a flywheel, slip recovery and
    burst correction on the GPU. Per block feed(nbits, bits) or feed_pipeline(pipe) after the pipeline's
    rds(); groups() returns that call's group records. Its own handle; the state stays on the device.
    soft_bits > 0 (or soft=True, for a soft handle at soft_bits 0) makes a handle of sdr_rds_dec_create_soft:
    feed then needs the tracker's soft row, and a failing block is first searched over its soft_bits least
    reliable raw decisions."""

    _destroy, _reset = "sdr_rds_dec_destroy", "sdr_rds_dec_reset"

    def __init__(self, nch: int, device: int = 0, max_burst: int = 2, loss_blocks: int = 8, soft_bits: int = 0,
                 soft: bool | None = None):
        h = C.c_void_p()
        self.soft = bool(soft_bits) if soft is None else bool(soft)
        if self.soft:
            so = rds_soft_opts(max_burst=max_burst, loss_blocks=loss_blocks, soft_bits=soft_bits)
            check(lib().sdr_rds_dec_create_soft(C.byref(h), device, nch, C.byref(so)), "sdr_rds_dec_create_soft")
        else:
            o = rds_opts(max_burst=max_burst, loss_blocks=loss_blocks)
            check(lib().sdr_rds_dec_create(C.byref(h), device, nch, C.byref(o)), "sdr_rds_dec_create")
        self._h = h
        self.nch, self.device = nch, device

    def feed(self, nbits, bits, stream=None, soft=None):
        """One call: nbits int32 [nch] and bits uint8 [nch][>= SDR_MAX_BITS] device tensors; soft: the uint16
        (or int16 storage) [nch][>= SDR_MAX_BITS] reliabilities of those bits, for a soft handle."""
        import torch
        if nbits.dtype != torch.int32 or tuple(nbits.shape) != (self.nch,) or not nbits.is_contiguous():
            raise ValueError(f"nbits must be a contiguous int32 [{self.nch}] tensor")
        if bits.dtype != torch.uint8 or bits.dim() != 2 or bits.shape[0] != self.nch or bits.shape[1] < SDR_MAX_BITS:
            raise ValueError(f"bits must be a uint8 [{self.nch}][>= {SDR_MAX_BITS}] tensor")
        if soft is not None:
            if soft.element_size() != 2 or soft.is_floating_point() or soft.dim() != 2 or soft.shape[0] != self.nch \
                    or soft.shape[1] < SDR_MAX_BITS:
                raise ValueError(f"soft must be a 16-bit integer [{self.nch}][>= {SDR_MAX_BITS}] tensor")
            check(lib().sdr_rds_groups_soft(self._h, _ptr(nbits), _ptr(bits), _row_stride(bits), _ptr(soft),
                                            _row_stride(soft), _stream(stream)), "sdr_rds_groups_soft")
            return
        check(lib().sdr_rds_groups(self._h, _ptr(nbits), _ptr(bits), _row_stride(bits), _stream(stream)),
              "sdr_rds_groups")

    def feed_pipeline(self, pipe: "Pipeline", stream=None):
        """The bits the pipeline's rds() / rds_bits() of the current block wrote (same stream)."""
        self.feed(pipe.nbits, pipe.bits, stream)

    def groups(self, stream=None):
        """(groups [nch][RDS_MAX_GROUPS] of rds_group_dtype(), counts int32 [nch]) of the last call;
        synchronises the stream."""
        import numpy as np
        g = np.zeros((self.nch, RDS_MAX_GROUPS), rds_group_dtype())
        n = np.zeros(self.nch, np.int32)
        check(lib().sdr_rds_groups_read(self._h, g.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p),
                                        _stream(stream)), "sdr_rds_groups_read")
        return g, n

    def stats(self, stream=None):
        """numpy structured array [nch] of rds_stats_dtype(); synchronises the stream."""
        return self._records("sdr_rds_stats_read", rds_stats_dtype(), stream)

    def soft_stats(self, stream=None):
        """numpy structured array [nch] of rds_soft_stats_dtype(); synchronises the stream."""
        return self._records("sdr_rds_soft_stats_read", rds_soft_stats_dtype(), stream)


def rds_track_stats_dtype():
    """numpy dtype of sdr_rds_track_stats (32 bytes)."""
    return _dtype(RdsTrackStats)


def rds_track_opts(**opts) -> RdsTrackOpts:
    """The tracker's defaults (sdr_rds_track_opts_default) with the given fields replaced."""
    return _opts(RdsTrackOpts, "sdr_rds_track_opts_default", "rds_track_opts", **opts)


class RdsTracker(_Handle):
    """The RDS symbol tracker of `nch` channels (sdr_rds_track_*): a bit clock carried from call to call and a
    biphase correlator over the whole bit, on the GPU. Per block feed(clean) or feed_pipeline(pipe) after the
    pipeline's rds(); the bits land in .nbits and .bits, in the layout RdsDecoder.feed takes. Mode 0 only.
    Its own handle; the state stays on the device."""

    _destroy, _reset = "sdr_rds_track_destroy", "sdr_rds_track_reset"

    def __init__(self, nch: int, device: int = 0, mode: int = 0, **opts):
        import torch
        h = C.c_void_p()
        o = rds_track_opts(**opts)
        check(lib().sdr_rds_track_create(C.byref(h), device, nch, mode, C.byref(o)), "sdr_rds_track_create")
        self._h = h
        self.nch, self.device = nch, device
        dev = torch.device("cuda", device)
        self.nbits = torch.zeros(nch, dtype=torch.int32, device=dev)
        self.bits = torch.zeros(nch, SDR_MAX_BITS, dtype=torch.uint8, device=dev)
        self.soft = None                 # the reliabilities of .bits, allocated by the first feed(..., soft=True)

    def feed(self, clean, n: int | None = None, stream=None, nbits=None, bits=None, soft=None):
        """One call: clean is a float32 [nch][>= n] device tensor of rds_clean rows (n: its row length by
        default); returns (nbits, bits), the tracker's own tensors unless others are given. soft: True for
        the tracker's own .soft (int16 storage of the u16 values, allocated on first use) or a 16-bit integer
        [nch][>= SDR_MAX_BITS] tensor; the call then also writes every bit's reliability and returns
        (nbits, bits, soft)."""
        import torch
        if clean.dtype != torch.float32 or clean.dim() != 2 or clean.shape[0] != self.nch:
            raise ValueError(f"clean must be a float32 [{self.nch}][n] tensor")
        n = int(clean.shape[1]) if n is None else int(n)
        if n > clean.shape[1]:
            raise ValueError(f"n {n} > the row length {clean.shape[1]}")
        nbits = self.nbits if nbits is None else nbits
        bits = self.bits if bits is None else bits
        if nbits.dtype != torch.int32 or tuple(nbits.shape) != (self.nch,) or not nbits.is_contiguous():
            raise ValueError(f"nbits must be a contiguous int32 [{self.nch}] tensor")
        if bits.dtype != torch.uint8 or bits.dim() != 2 or bits.shape[0] != self.nch or bits.shape[1] < SDR_MAX_BITS:
            raise ValueError(f"bits must be a uint8 [{self.nch}][>= {SDR_MAX_BITS}] tensor")
        if soft is not None and soft is not False:
            if soft is True:
                if self.soft is None:
                    self.soft = torch.zeros(self.nch, SDR_MAX_BITS, dtype=torch.int16, device=bits.device)
                soft = self.soft
            if soft.element_size() != 2 or soft.is_floating_point() or soft.dim() != 2 or soft.shape[0] != self.nch \
                    or soft.shape[1] < SDR_MAX_BITS:
                raise ValueError(f"soft must be a 16-bit integer [{self.nch}][>= {SDR_MAX_BITS}] tensor")
            check(lib().sdr_rds_track_bits_soft(self._h, _ptr(clean), _row_stride(clean), n, _ptr(nbits), _ptr(bits),
                                                _row_stride(bits), _ptr(soft), _row_stride(soft), _stream(stream)),
                  "sdr_rds_track_bits_soft")
            return nbits, bits, soft
        check(lib().sdr_rds_track_bits(self._h, _ptr(clean), _row_stride(clean), n, _ptr(nbits), _ptr(bits), _row_stride(bits),
                                       _stream(stream)), "sdr_rds_track_bits")
        return nbits, bits

    def feed_pipeline(self, pipe: "Pipeline", clean, stream=None):
        """The rds_clean rows the pipeline's rds() of the current block returned (same stream)."""
        return self.feed(clean, pipe.info.n_rds, stream)

    def stats(self, stream=None):
        """numpy structured array [nch] of rds_track_stats_dtype(); synchronises the stream."""
        return self._records("sdr_rds_track_stats_read", rds_track_stats_dtype(), stream)


def rds_carrier_stats_dtype():
    """numpy dtype of sdr_rds_carrier_stats (40 bytes)."""
    return _dtype(RdsCarrierStats)


def rds_carrier_opts(**opts) -> RdsCarrierOpts:
    """The derotator's defaults (sdr_rds_carrier_opts_default) with the given fields replaced."""
    return _opts(RdsCarrierOpts, "sdr_rds_carrier_opts_default", "rds_carrier_opts", **opts)


def rds_carrier_phase_deg(stats):
    """The phase in use in degrees, of records of rds_carrier_stats_dtype()."""
    import numpy as np
    return np.asarray(stats["phi"], np.float64) * (360.0 / 2.0 ** 32)


def rds_carrier_coherence(stats):
    """hypot(sr, si) / st of records of rds_carrier_stats_dtype(): 1 for a clean BPSK subcarrier, near 0 for
    noise, 0 before the first window."""
    import numpy as np
    st = np.asarray(stats["st"], np.float64)
    h = np.hypot(np.asarray(stats["sr"], np.float64), np.asarray(stats["si"], np.float64))
    return np.divide(h, st, out=np.zeros_like(h), where=st > 0)


class RdsCarrier(_Handle):
    """The RDS carrier-phase derotator of `nch` channels (sdr_rds_carrier_*): per call it turns the in-phase and
    quadrature rds_clean rows onto one axis by the phase of their squared signal, estimated window by window of
    the stream, on the GPU. feed(clean_i, clean_q) returns rows that RdsTracker.feed takes in place of rds_clean.
    Mode 0 only. Its own handle; the state stays on the device."""

    _destroy, _reset = "sdr_rds_carrier_destroy", "sdr_rds_carrier_reset"

    def __init__(self, nch: int, device: int = 0, mode: int = 0, **opts):
        h = C.c_void_p()
        o = rds_carrier_opts(**opts)
        check(lib().sdr_rds_carrier_create(C.byref(h), device, nch, mode, C.byref(o)), "sdr_rds_carrier_create")
        self._h = h
        self.nch, self.device = nch, device
        self.out = None                  # the rotated rows, allocated by the first feed() that is given none

    def feed(self, clean_i, clean_q, n: int | None = None, stream=None, out=None):
        """One call: clean_i and clean_q are float32 [nch][>= n] device tensors (n: the shorter row length by
        default); returns the rotated rows, float32 [nch][>= n]: `out`, or the handle's own tensor, which the
        next call overwrites."""
        import torch
        for name, x in (("clean_i", clean_i), ("clean_q", clean_q)):
            if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != self.nch:
                raise ValueError(f"{name} must be a float32 [{self.nch}][n] tensor")
        n = int(min(clean_i.shape[1], clean_q.shape[1])) if n is None else int(n)
        if n > min(clean_i.shape[1], clean_q.shape[1]):
            raise ValueError(f"n {n} > a row's length")
        if out is None:
            if self.out is None or self.out.shape[1] < n:
                self.out = torch.zeros(self.nch, max(n, 1), dtype=torch.float32, device=clean_i.device)
            out = self.out
        if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != self.nch or out.shape[1] < n:
            raise ValueError(f"out must be a float32 [{self.nch}][>= {n}] tensor")
        check(lib().sdr_rds_carrier_rotate(self._h, _ptr(clean_i), _row_stride(clean_i), _ptr(clean_q), _row_stride(clean_q),
                                           n, _ptr(out), _row_stride(out), _stream(stream)), "sdr_rds_carrier_rotate")
        return out

    def feed_pipeline(self, pipe: "Pipeline", clean, stream=None, out=None):
        """The rds_clean rows a RDS_QUAD pipeline's rds() or rds_post() of the current block returned, with the
        context's own rds_clean_q rows where they are (same stream, no copy); returns the rotated rows."""
        import torch
        p, s, n = C.c_void_p(), C.c_size_t(), C.c_int()
        check(lib().sdr_ctx_rds_clean_q(pipe._h, C.byref(p), C.byref(s), C.byref(n)), "sdr_ctx_rds_clean_q")
        if clean.dtype != torch.float32 or clean.dim() != 2 or clean.shape[0] != self.nch or clean.shape[1] < n.value:
            raise ValueError(f"clean must be a float32 [{self.nch}][>= {n.value}] tensor")
        if out is None:
            if self.out is None or self.out.shape[1] < n.value:
                self.out = torch.zeros(self.nch, n.value, dtype=torch.float32, device=clean.device)
            out = self.out
        if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != self.nch or out.shape[1] < n.value:
            raise ValueError(f"out must be a float32 [{self.nch}][>= {n.value}] tensor")
        check(lib().sdr_rds_carrier_rotate(self._h, _ptr(clean), _row_stride(clean), p, s.value, n.value, _ptr(out),
                                           _row_stride(out), _stream(stream)), "sdr_rds_carrier_rotate")
        return out

    def stats(self, stream=None):
        """numpy structured array [nch] of rds_carrier_stats_dtype(); synchronises the stream."""
        return self._records("sdr_rds_carrier_stats_read", rds_carrier_stats_dtype(), stream)


class RdsStation:
    """The text layer of one station (sdr_rds_station_*, host only): update(groups) with records of
    rds_group_dtype(), text() for the report; the fields are on .s (RdsStationC)."""

    def __init__(self):
        self.s = RdsStationC()
        lib().sdr_rds_station_init(C.byref(self.s))

    def update(self, groups):
        import numpy as np
        a = np.ascontiguousarray(np.atleast_1d(np.asarray(groups, rds_group_dtype())).reshape(-1))
        base = a.ctypes.data
        for k in range(a.shape[0]):
            lib().sdr_rds_station_update(C.byref(self.s), C.cast(base + 16 * k, C.POINTER(RdsGroup)))

    def set_stats(self, stats):
        """One channel's counters (a record of rds_stats_dtype()) for the block error rate."""
        import numpy as np
        a = np.ascontiguousarray(np.asarray(stats, rds_stats_dtype()).reshape(-1)[:1])
        lib().sdr_rds_station_stats(C.byref(self.s), C.cast(a.ctypes.data, C.POINTER(RdsStats)))

    @property
    def pi(self):
        return int(self.s.pi) if self.s.pi_valid else None

    @property
    def ps(self):
        return bytes(self.s.ps_done).decode("latin-1") if self.s.ps_complete else None

    @property
    def af_mhz(self):
        return [self.s.af[i] / 10.0 for i in range(min(self.s.af_n, 25))]

    def bler(self) -> float:
        return float(lib().sdr_rds_station_bler(C.byref(self.s)))

    def text(self) -> str:
        buf = C.create_string_buffer(2048)
        lib().sdr_rds_station_format(C.byref(self.s), buf, len(buf))
        return buf.value.decode("ascii", errors="replace")


# ------------------------------------------------------------------ batched primitives (torch tensors)
def convolve_fir(y, x, h, state, D: int, stream=None):
    """convolveFIR(y, x, h, state, D) for every row: y[nch][nx/D], x[nch][nx], state[nch][>=ntaps-1]."""
    nch, nx = x.shape
    check(lib().sdr_convolve_fir(_ptr(y), _row_stride(y), _ptr(x), _row_stride(x), nch, nx, _ptr(h), h.numel(),
                                 _ptr(state), state.shape[1], D, _stream(stream)), "convolve_fir")
    return y


def convolve_fir_resample(y, x, h, state, U: int, D: int, stream=None):
    """convolveFIR(y, x, h, state, U, D) for every row: y[nch][nx*U/D]."""
    nch, nx = x.shape
    check(lib().sdr_convolve_fir_resample(_ptr(y), _row_stride(y), _ptr(x), _row_stride(x), nch, nx, _ptr(h),
                                          h.numel(), _ptr(state), state.shape[1], U, D, _stream(stream)),
          "convolve_fir_resample")
    return y


def fm_demod(out, I, Q, prev, stream=None):
    """fmDemodNoArctan for every row; prev[nch][2] = (prev_I, prev_Q), updated in place."""
    nch, n = I.shape
    assert Q.stride(0) == I.stride(0)
    check(lib().sdr_fm_demod(_ptr(out), _row_stride(out), _ptr(I), _ptr(Q), _row_stride(I), nch, n, _ptr(prev),
                             _stream(stream)), "fm_demod")
    return out


def fm_demod_phase(out, I, Q, prev, stream=None):
    """The phase discriminator (PHASE_DEMOD, include/sdr_amd.h) for every row: the phase step in radians;
    prev[nch][2] = (prev_I, prev_Q), updated in place."""
    nch, n = I.shape
    assert Q.stride(0) == I.stride(0)
    check(lib().sdr_fm_demod_phase(_ptr(out), _row_stride(out), _ptr(I), _ptr(Q), _row_stride(I), nch, n, _ptr(prev),
                                   _stream(stream)), "fm_demod_phase")
    return out


def demod_coeffs():
    """c_0 .. c_K of the phase discriminator's odd polynomial (sdr_demod_coeffs, host only)."""
    import numpy as np
    n = C.c_int(0)
    check(lib().sdr_demod_coeffs(None, 0, C.byref(n)), "sdr_demod_coeffs")
    c = np.zeros(n.value, np.float32)
    check(lib().sdr_demod_coeffs(c.ctypes.data_as(C.c_void_p), c.size, C.byref(n)), "sdr_demod_coeffs")
    return c


def fmpll(out, x, freq, Fs, state, ncoScale=1.0, phaseAdjust=0.0, normBandwidth=0.01, stream=None):
    """fmpll for every row: out[nch][n+1]; state = uint8 tensor holding nch PllState records."""
    nch, n = x.shape
    check(lib().sdr_fmpll(_ptr(out), _row_stride(out), _ptr(x), _row_stride(x), nch, n, freq, Fs, _ptr(state),
                          ncoScale, phaseAdjust, normBandwidth, _stream(stream)), "fmpll")
    return out


def cdr(offset, x, sps: int, stream=None):
    nch, n = x.shape
    check(lib().sdr_cdr(_ptr(offset), _ptr(x), _row_stride(x), nch, n, sps, _stream(stream)), "cdr")
    return offset


def manchester_decode(bits, nbits, symbols, nsym, block_count: int, state, stream=None):
    """manchester_decode for every row: symbols[nch][>= nsym[ch]] 0/1 uint8, nsym[nch] int32,
    state[nch][2] int32 = {half_symbol, start} updated in place; bits[nch][>= nsym/2 + 1] uint8 and
    nbits[nch] int32 are written. A row with nsym <= 0 gets nbits = 0 and nothing else."""
    nch = symbols.shape[0]
    check(lib().sdr_manchester_decode(_ptr(bits), _row_stride(bits), _ptr(nbits), _ptr(symbols), _row_stride(symbols),
                                      _ptr(nsym), nch, block_count, _ptr(state), _stream(stream)), "manchester_decode")
    return bits


def differential_decode(out, bits, nbits, block_num: int, last_bit, stream=None):
    """differential_decode for every row: bits[nch][>= nbits[ch]] uint8, nbits[nch] int32, last_bit[nch]
    int32 updated in place; out[nch][>= nbits[ch]] uint8. Rows with nbits <= 0 are left untouched."""
    nch = bits.shape[0]
    check(lib().sdr_differential_decode(_ptr(out), _row_stride(out), _ptr(bits), _row_stride(bits), _ptr(nbits), nch,
                                        block_num, _ptr(last_bit), _stream(stream)), "differential_decode")
    return out


def pll_state_tensor(nch: int, device="cuda", feedbackI=1.0, lastCarrier=1.0):
    """Device array of nch PllState records initialised like stereo.cpp:51-57."""
    import numpy as np
    import torch
    arr = (PllState * nch)()
    for i in range(nch):
        arr[i] = PllState(feedbackI, 0.0, 0.0, 0.0, 0.0, lastCarrier)
    raw = np.frombuffer(bytes(arr), dtype=np.uint8).copy()
    return torch.from_numpy(raw).to(device)


def pll_state_from_tensor(t) -> list:
    raw = t.cpu().numpy().tobytes()
    n = len(raw) // C.sizeof(PllState)
    arr = (PllState * n).from_buffer_copy(raw)
    return list(arr)


# ------------------------------------------------------------------ fused pipeline
class Pipeline(_Handle):
    """A device context of `nch` channels: the reference's RF_frontend + mono + stereo + rds bodies.

    Per block: frontend(iq) then any of mono(), stereo(), rds() (each at most once per block).
    """

    _destroy, _reset = "sdr_ctx_destroy", "sdr_ctx_reset"

    def __init__(self, nch: int, mode: int = 0, rds_on: bool = True, device: int = 0, flags: int = 0):
        import torch
        self.device = device
        self.torch_device = torch.device("cuda", device)
        h = C.c_void_p()
        check(lib().sdr_ctx_create(C.byref(h), device, nch, mode, 1 if rds_on else 0, flags), "sdr_ctx_create")
        self._h = h
        info = Info()
        check(lib().sdr_ctx_info(self._h, C.byref(info)), "sdr_ctx_info")
        self.info = info
        self.nch = nch
        self.flags = flags
        i32 = torch.int32
        dev = self.torch_device
        self.offset = torch.zeros(nch, dtype=i32, device=dev)
        self.nsym = torch.zeros(nch, dtype=i32, device=dev)
        self.nbits = torch.zeros(nch, dtype=i32, device=dev)
        self.symbols = torch.zeros(nch, SDR_MAX_SYMS, dtype=torch.uint8, device=dev)
        self.bits = torch.zeros(nch, SDR_MAX_BITS, dtype=torch.uint8, device=dev)

    def frontend(self, iq, stream=None):
        """iq: uint8 [nch][2*block_iq] (device)."""
        check(lib().sdr_frontend(self._h, _ptr(iq), _row_stride(iq), _stream(stream)), "sdr_frontend")

    # shared-capture tuner (include/sdr_amd.h): channel ch = row src[ch] of the capture batch, shifted by khz[ch]
    def set_tuning(self, src, khz, nsrc=None, stream=None):
        """Tune the context (only at block 0): src, khz are [nch] integer sequences; nsrc defaults to
        max(src) + 1. frontend_tuned(iq [nsrc][2*block_iq]) then replaces frontend()."""
        import numpy as np
        src = np.ascontiguousarray(src, np.int32)
        khz = np.ascontiguousarray(khz, np.int32)
        if src.shape != (self.nch,) or khz.shape != (self.nch,):
            raise SdrError(f"set_tuning: src and khz must have {self.nch} entries", -1)
        if nsrc is None:
            nsrc = int(src.max()) + 1
        check(lib().sdr_tuner_set(self._h, int(nsrc), src.ctypes.data_as(C.c_void_p), khz.ctypes.data_as(C.c_void_p),
                                  _stream(stream)), "sdr_tuner_set")

    def clear_tuning(self, stream=None):
        check(lib().sdr_tuner_set(self._h, 0, None, None, _stream(stream)), "sdr_tuner_set")

    @property
    def nsrc(self) -> int:
        """Source rows of the tuning, 0: not tuned."""
        n = C.c_int(0)
        check(lib().sdr_tuner_get(self._h, C.byref(n)), "sdr_tuner_get")
        return n.value

    def frontend_tuned(self, iq, stream=None):
        """iq: uint8 [nsrc][2*block_iq] (device), the capture rows of a tuned context."""
        # (a single row's stride is never used, and a view of one may report any)
        stride = _row_stride(iq) if iq.shape[0] > 1 else int(iq.shape[1])
        check(lib().sdr_frontend_tuned(self._h, _ptr(iq), stride, _stream(stream)), "sdr_frontend_tuned")

    def release_wait(self, stream=None):
        """The parity-release wait of the next frontend(), enqueued now on `stream` (that call then
        enqueues none there): the front-end kernel can be timed alone."""
        check(lib().sdr_frontend_release_wait(self._h, _stream(stream)), "sdr_frontend_release_wait")

    def frontend_timing(self, max_launches: int):
        """Record the dispatch start / end of the next max_launches frontend() kernels."""
        check(lib().sdr_frontend_timing(self._h, max_launches), "sdr_frontend_timing")

    def frontend_times(self, max_launches: int = 4096) -> list:
        """ms per timed frontend() kernel, in call order (synchronises with the last)."""
        arr = (C.c_double * max_launches)()
        n = C.c_int(0)
        check(lib().sdr_frontend_times(self._h, arr, max_launches, C.byref(n)), "sdr_frontend_times")
        return list(arr[:n.value])

    def frontend_stamps(self, max_launches: int = 4096) -> tuple[list, list]:
        """(start, end) of each timed frontend() kernel in 100 MHz device ticks (plls_timeline's clock)."""
        a, z = (C.c_ulonglong * max_launches)(), (C.c_ulonglong * max_launches)()
        n = C.c_int(0)
        check(lib().sdr_frontend_stamps(self._h, a, z, max_launches, C.byref(n)), "sdr_frontend_stamps")
        return list(a[:n.value]), list(z[:n.value])

    def fm_demod(self, out=None, stream=None):
        import torch
        if out is None:
            out = torch.empty(self.nch, self.info.block_if, dtype=torch.float32, device=self.torch_device)
        check(lib().sdr_get_fm_demod(self._h, _ptr(out), _row_stride(out), _stream(stream)), "sdr_get_fm_demod")
        return out

    def mono(self, out=None, stream=None):
        import torch
        if out is None:
            out = torch.empty(self.nch, self.info.n_audio, dtype=torch.int16, device=self.torch_device)
        check(lib().sdr_mono(self._h, _ptr(out), _row_stride(out), _stream(stream)), "sdr_mono")
        return out

    def stereo(self, out=None, stream=None):
        import torch
        if out is None:
            out = torch.empty(self.nch, 2 * self.info.n_audio, dtype=torch.int16, device=self.torch_device)
        check(lib().sdr_stereo(self._h, _ptr(out), _row_stride(out), _stream(stream)), "sdr_stereo")
        return out

    # the stereo / RDS bodies split at their PLL (include/sdr_amd.h): pre; pll; post per block
    def stereo_pre(self, stream=None):
        check(lib().sdr_stereo_pre(self._h, _stream(stream)), "sdr_stereo_pre")

    def stereo_pll(self, stream=None):
        check(lib().sdr_stereo_pll(self._h, _stream(stream)), "sdr_stereo_pll")

    def stereo_post(self, out, stream=None):
        check(lib().sdr_stereo_post(self._h, _ptr(out), _row_stride(out), _stream(stream)), "sdr_stereo_post")
        return out

    def rds_pre(self, stream=None):
        check(lib().sdr_rds_pre(self._h, _stream(stream)), "sdr_rds_pre")

    def pre(self, stream=None):
        """stereo_pre + rds_pre on one stream, the three fm_demod BPFs sharing one staged window."""
        check(lib().sdr_pre(self._h, _stream(stream)), "sdr_pre")

    def rds_pll(self, stream=None):
        check(lib().sdr_rds_pll(self._h, _stream(stream)), "sdr_rds_pll")

    def plls(self, stream=None):
        """stereo_pll + rds_pll in one dispatch."""
        check(lib().sdr_plls(self._h, _stream(stream)), "sdr_plls")

    # persistent PLLs (include/sdr_amd.h): one dispatch for many blocks
    def plls_launch(self, nblocks: int, stream=None, which: int = 3):
        """Persistent PLLs of the next nblocks blocks (which = 3: both; 1: stereo, 2: RDS only)."""
        check(lib().sdr_plls_launch_sel(self._h, nblocks, which, _stream(stream)), "sdr_plls_launch_sel")

    def plls_fits(self, n_cu: int, first_cu: int = 0, which: int = 3) -> dict:
        """Would plls_launch (which = 3: both PLLs; 1 stereo, 2 RDS: plls_launch_sel) accept a stream
        over CUs [first_cu, first_cu + n_cu)? The launch's waves, workgroups and how many of those the
        range keeps resident at once (sdr_plls_fits)."""
        w, g, r = C.c_int(), C.c_longlong(), C.c_longlong()
        check(lib().sdr_plls_fits(self._h, which, first_cu, n_cu, C.byref(w), C.byref(g), C.byref(r)),
              "sdr_plls_fits")
        return {"waves": w.value, "groups": g.value, "resident": r.value, "fits": g.value <= r.value}

    def plls_plan(self, n_cu: int, first_cu: int = 0, which: int = 3) -> dict:
        """Which kernel plls_launch(which) takes on a stream over CUs [first_cu, first_cu + n_cu)
        (sdr_diag_plls_plan; nothing is enqueued): waves per workgroup, whether it is the LDS-staged
        lane-pair loop, whether the trigArg table fits LDS (the TAB = true kernels), and the
        launch's dynamic LDS bytes."""
        out = (C.c_int * 4)()
        check(lib().sdr_diag_plls_plan(self._h, which, first_cu, n_cu, out), "sdr_diag_plls_plan")
        return {"wg_waves": out[0], "staged": bool(out[1]), "tab_ok": out[2], "lds": out[3]}

    def plls_prepare(self, nblocks: int, stream=None):
        """The launch's bookkeeping ahead of plls_launch(nblocks) (allocation, stamp reset)."""
        check(lib().sdr_plls_prepare(self._h, nblocks, _stream(stream)), "sdr_plls_prepare")

    def plls_signal(self, stream=None):
        check(lib().sdr_plls_signal(self._h, _stream(stream)), "sdr_plls_signal")

    def frontend_pre_parts(self, iq, nparts: int, stream=None):
        """The first block of a pending persistent launch: frontend + pre + plls_signal in nparts
        sample ranges, each published to the PLLs as soon as it is ready (the pipeline fill)."""
        check(lib().sdr_frontend_pre_parts(self._h, _ptr(iq), _row_stride(iq), nparts, _stream(stream)),
              "sdr_frontend_pre_parts")

    def plls_wait(self, stream=None):
        check(lib().sdr_plls_wait(self._h, _stream(stream)), "sdr_plls_wait")

    def plls_report(self, max_blocks: int = 4096, stream=None) -> list:
        """Per-block PLL time (ms) of the last persistent launch; raises if a wait timed out."""
        arr = (C.c_double * max_blocks)()
        n = C.c_int(0)
        check(lib().sdr_plls_report(self._h, arr, max_blocks, C.byref(n), _stream(stream)), "sdr_plls_report")
        return list(arr[:n.value])

    def plls_timeline(self, max_blocks: int = 4096, stream=None) -> tuple[list, list]:
        """(t_start, t_end) per block of the last persistent launch, 100 MHz device ticks."""
        a, z = (C.c_ulonglong * max_blocks)(), (C.c_ulonglong * max_blocks)()
        n = C.c_int(0)
        check(lib().sdr_plls_timeline(self._h, a, z, max_blocks, C.byref(n), _stream(stream)), "sdr_plls_timeline")
        return list(a[:n.value]), list(z[:n.value])

    def plls_cycles(self, stream=None) -> tuple[float, float]:
        """(shader cycles per PLL step and wave, shader clock MHz) of the last persistent launch."""
        cyc, mhz = C.c_double(0.0), C.c_double(0.0)
        check(lib().sdr_plls_cycles(self._h, C.byref(cyc), C.byref(mhz), _stream(stream)), "sdr_plls_cycles")
        return cyc.value, mhz.value

    def plls_block_cycles(self, stream=None, max_blocks: int = 4096) -> tuple[list, list]:
        """Per block of the last persistent launch: (cycles per step and wave, shader clock MHz)."""
        cyc, mhz = (C.c_double * max_blocks)(), (C.c_double * max_blocks)()
        n = C.c_int(0)
        check(lib().sdr_plls_block_cycles(self._h, cyc, mhz, max_blocks, C.byref(n), _stream(stream)),
              "sdr_plls_block_cycles")
        k = min(n.value, max_blocks)
        return list(cyc[:k]), list(mhz[:k])

    def rds_post(self, out=None, bits=True, stream=None, bits_out=None):
        """bits_out: a [nch][SDR_MAX_BITS] u8 tensor the block's bits go to instead of self.bits."""
        check(lib().sdr_rds_post(self._h, _ptr(out), _row_stride(out) if out is not None else 0, _stream(stream)),
              "sdr_rds_post")
        if bits:
            self.rds_bits(stream, bits_out)
        return out

    def rds_bits(self, stream=None, bits_out=None):
        b = self.bits if bits_out is None else bits_out
        if tuple(b.shape) != (self.nch, SDR_MAX_BITS) or b.dtype != self.bits.dtype or not b.is_contiguous():
            raise ValueError(f"bits_out must be a contiguous [{self.nch}][{SDR_MAX_BITS}] uint8 tensor")
        check(lib().sdr_rds_bits(self._h, _ptr(self.offset), _ptr(self.nsym), _ptr(self.symbols), SDR_MAX_SYMS,
                                 _ptr(self.nbits), _ptr(b), SDR_MAX_BITS, _stream(stream)), "sdr_rds_bits")

    def push_fm_demod(self, fm, stream=None):
        """Make fm [nch][block_if] (device f32) the current block (the queue's consumer side)."""
        check(lib().sdr_push_fm_demod(self._h, _ptr(fm), _row_stride(fm), _stream(stream)), "sdr_push_fm_demod")

    def rds(self, out=None, bits=True, stream=None):
        """RDS DSP (+ symbol/bit recovery). Returns rds_clean [nch][n_rds]; bits in self.bits/nbits."""
        import torch
        if out is None:
            out = torch.empty(self.nch, self.info.n_rds, dtype=torch.float32, device=self.torch_device)
        check(lib().sdr_rds_dsp(self._h, _ptr(out), _row_stride(out), _stream(stream)), "sdr_rds_dsp")
        if bits:
            check(lib().sdr_rds_bits(self._h, _ptr(self.offset), _ptr(self.nsym), _ptr(self.symbols),
                                     SDR_MAX_SYMS, _ptr(self.nbits), _ptr(self.bits), SDR_MAX_BITS,
                                     _stream(stream)), "sdr_rds_bits")
        return out

    def rds_clean_q(self, out=None, stream=None):
        """The quadrature branch's rows of the current block (a RDS_QUAD pipeline, after rds() or rds_post()),
        copied on `stream` into out [nch][>= n_rds] (a new tensor by default) without a synchronisation: what
        RdsCarrier.feed takes beside rds_clean."""
        import ctypes
        import torch
        p, s, n = C.c_void_p(), C.c_size_t(), C.c_int()
        check(lib().sdr_ctx_rds_clean_q(self._h, C.byref(p), C.byref(s), C.byref(n)), "sdr_ctx_rds_clean_q")
        if out is None:
            out = torch.empty(self.nch, n.value, dtype=torch.float32, device=self.torch_device)
        if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != self.nch or out.shape[1] < n.value:
            raise ValueError(f"out must be a float32 [{self.nch}][>= {n.value}] tensor")
        rc = _hip().hipMemcpy2DAsync(ctypes.c_void_p(out.data_ptr()), ctypes.c_size_t(4 * _row_stride(out)), p,
                                     ctypes.c_size_t(4 * s.value), ctypes.c_size_t(4 * n.value),
                                     ctypes.c_size_t(self.nch), ctypes.c_int(3), ctypes.c_void_p(_stream(stream)))
        if rc != 0:
            raise SdrError(f"hipMemcpy2DAsync failed ({rc})")
        return out

    def buffer(self, name: str, stream=None):
        """Current-block intermediate copied into a new [nch][len] tensor (on `stream`, which is then
        synchronised; the default is the legacy null stream, which waits for every blocking stream
        -- never use it while a persistent PLL launch still waits for blocks)."""
        import torch
        p, s, n = C.c_void_p(), C.c_size_t(), C.c_int()
        check(lib().sdr_ctx_buffer(self._h, name.encode(), C.byref(p), C.byref(s), C.byref(n)), "sdr_ctx_buffer")
        full = torch.empty(0, dtype=torch.float32, device=self.torch_device)
        # wrap the device pointer through a DLPack-free path: copy rows with cudaMemcpy2D via torch
        out = torch.empty(self.nch, n.value, dtype=torch.float32, device=self.torch_device)
        import ctypes
        hip = _hip()
        st = _stream(stream) if stream is not None else None
        if st is None:
            rc = hip.hipMemcpy2D(ctypes.c_void_p(out.data_ptr()), ctypes.c_size_t(4 * n.value), p,
                                 ctypes.c_size_t(4 * s.value), ctypes.c_size_t(4 * n.value),
                                 ctypes.c_size_t(self.nch), ctypes.c_int(3))
        else:
            rc = hip.hipMemcpy2DAsync(ctypes.c_void_p(out.data_ptr()), ctypes.c_size_t(4 * n.value), p,
                                      ctypes.c_size_t(4 * s.value), ctypes.c_size_t(4 * n.value),
                                      ctypes.c_size_t(self.nch), ctypes.c_int(3), ctypes.c_void_p(st))
            if rc == 0:
                rc = hip.hipStreamSynchronize(ctypes.c_void_p(st))
        if rc != 0:
            raise SdrError(f"hipMemcpy2D failed ({rc})")
        del full
        return out


_hiplib = None


def _hip():
    global _hiplib
    if _hiplib is None:
        import ctypes.util
        for cand in ("libamdhip64.so", "libamdhip64.so.7", "/opt/rocm/lib/libamdhip64.so"):
            try:
                _hiplib = C.CDLL(cand)
                break
            except OSError:
                continue
        if _hiplib is None:
            raise SdrError("libamdhip64.so not found")
        _hiplib.hipMemcpy2D.restype = C.c_int
        _hiplib.hipMemcpy2DAsync.restype = C.c_int
        _hiplib.hipMemcpyAsync.restype = C.c_int
        _hiplib.hipStreamSynchronize.restype = C.c_int
    return _hiplib
