"""ctypes binding of libgypsum_hip.so (include/gypsum_hip.h).  Fails loudly if the library is missing."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

import os

# GYPSUM_HIP_LIB points at an alternative build of the same library (A/B experiments); default: the in-tree one
LIB_PATH = Path(os.environ.get("GYPSUM_HIP_LIB") or Path(__file__).resolve().parent / "csrc" / "libgypsum_hip.so")

GYP_OK = 0
GYP_E_BAD_ARG, GYP_E_BAD_RATE, GYP_E_NO_DEVICE, GYP_E_HIP, GYP_E_NO_FORMAT, GYP_E_NOMEM, GYP_E_IO = -1, -2, -3, -4, -5, -6, -7
GYP_FMT_F32, GYP_FMT_I8, GYP_FMT_I16, GYP_FMT_U8 = 0, 1, 2, 3
GYP_COHERENT, GYP_NON_COHERENT = 0, 1

# numpy mirrors of the C records (layouts asserted against the header in tests/test_abi.py)
CELL_DESC = np.dtype([("stream", "<i4"), ("sat_id", "<i4"), ("doppler_hz", "<f8"), ("tap_index", "<i4"),
                      ("reserved", "<i4")], align=True)
CELL = np.dtype([("peak", "<f4"), ("argmax", "<i4"), ("sum", "<f8"), ("n_max", "<i4"), ("reserved", "<i4"),
                 ("tap_re", "<f4"), ("tap_im", "<f4")], align=True)
ACQ_RESULT = np.dtype([("stream", "<i4"), ("sat_id", "<i4"), ("doppler_hz", "<i4"), ("code_phase", "<i4"),
                       ("carrier_phase", "<f8"), ("strength", "<f8")], align=True)
CHAN_IN = np.dtype([("stream", "<i4"), ("sat_id", "<i4"), ("doppler_hz", "<f8"), ("carrier_phase", "<f8"),
                    ("code_phase", "<i4"), ("reserved", "<i4")], align=True)
CHAN_OUT = np.dtype([("early_re", "<f4"), ("early_im", "<f4"), ("late_re", "<f4"), ("late_im", "<f4"),
                     ("peak_re", "<f4"), ("peak_im", "<f4"), ("peak_mag", "<f4"), ("peak_offset", "<i4"),
                     ("sum", "<f8"), ("n_max", "<i4"), ("reserved", "<i4"),
                     ("early64_re", "<f8"), ("early64_im", "<f8"), ("late64_re", "<f8"), ("late64_im", "<f8")], align=True)
BEST_BIN = np.dtype([("bin", "<i4"), ("argmax", "<i4"), ("peak", "<f4"), ("reserved", "<i4"), ("strength", "<f8")], align=True)
CHAN_INIT = CHAN_IN
PARAMS = np.dtype([(k, "<f8") for k in (
    "acq_initial_spread_hz", "acq_min_spread_hz", "acq_bins_per_spread", "dll_gain", "dll_phase_modulus",
    "pll_bandwidth_locked_hz", "pll_bandwidth_unlocked_hz", "lock_error_variance_max", "lock_i_variance_max",
    "lock_rotation_max_deg", "watchdog_period_s", "watchdog_drop_below", "watchdog_nudge_below", "watchdog_nudge_hz",
    "spec_confidence_kappa", "acq_reuse_level_records")], align=True)
TRACK_REC = np.dtype([("peak_re", "<f4"), ("peak_im", "<f4"), ("strength", "<f4"), ("discriminator", "<f4"),
                      ("doppler_hz", "<f8"), ("carrier_phase", "<f8"), ("error", "<f8"), ("code_phase", "<i4"),
                      ("peak_offset", "<i4"), ("pseudosymbol", "i1"), ("locked", "i1"), ("status", "i1"),
                      ("nudged", "i1"), ("path_info", "<i4")], align=True)
SYNTH_SAT = np.dtype([("sat_id", "<i4"), ("code_phase", "<i4"), ("doppler_hz", "<f8"), ("carrier_phase", "<f8"),
                      ("amplitude", "<f4"), ("nav_bit_offset_ms", "<i4")], align=True)
BIT_EVENT = np.dtype([("receiver_timestamp", "<f8"), ("trailing_edge_receiver_timestamp", "<f8"), ("channel", "<i4"),
                      ("bit_value", "<i4")], align=True)
BITS_STATE = np.dtype([("determined_bit_phase", "<i4"), ("previous_bit_phase_decision", "<i4"),
                       ("sequential_unknown_bit_value_counter", "<i4"), ("queued_pseudosymbols", "<i4"),
                       ("pseudosymbol_cursor_within_queue", "<i8"), ("slide", "<i8"), ("failed_bit_count", "<i8"),
                       ("emitted_bit_count", "<i8"), ("processed_pseudosymbol_count", "<i8"),
                       ("last_emitted_bits_len", "<i4"), ("last_emitted_bits", "i1", (52,))], align=True)
PACKING = np.dtype([("bits", "<i4"), ("real", "<i4"), ("order", "<i4"), ("reserved", "<i4"), ("levels", "<f4", (16,))], align=True)
GYP_PACK_MSB_FIRST, GYP_PACK_LSB_FIRST = 0, 1
IQ_STATS = np.dtype([("sum_re", "<f8"), ("sum_im", "<f8"), ("sum_sq", "<f8"), ("max_abs", "<f4"), ("n_clip", "<i4")], align=True)
IQ_LEVEL = np.dtype([("dc_re", "<f4"), ("dc_im", "<f4"), ("gain", "<f4"), ("reserved", "<i4")], align=True)
TONE_REC = np.dtype([("re", "<f8"), ("im", "<f8")], align=True)
NOTCH_TONES = np.dtype([("count", "<i4"), ("reserved", "<i4"), ("freq_hz", "<i8", (8,))], align=True)
QUALITY_SUMS = np.dtype([("n_used", "<i4"), ("n_locked", "<i4"), ("n_groups", "<i4"), ("reserved", "<i4"), ("sum_p2", "<f8"),
                         ("sum_p4", "<f8"), ("sum_np", "<f8"), ("sum_pl", "<f8")], align=True)
QUALITY = np.dtype([("cn0_m2m4_dbhz", "<f8"), ("cn0_nwpr_dbhz", "<f8"), ("phase_lock", "<f8"), ("locked_share", "<f8"),
                    ("n_used", "<i4"), ("n_groups", "<i4")], align=True)
BLANKER = np.dtype([("center_re", "<f4"), ("center_im", "<f4"), ("threshold", "<f4"), ("guard", "<i4")], align=True)
EXCISOR = np.dtype([("threshold", "<f4"), ("guard", "<i4"), ("reserved", "<i4", (2,))], align=True)
HYBRID_CELL = np.dtype([("peak", "<f4"), ("argmax", "<i4"), ("second", "<f4"), ("second_argmax", "<i4"), ("n_off", "<i4"), ("set", "<i4"),
                        ("sum_off", "<f8"), ("sumsq_off", "<f8"), ("blocks_used", "<i4"), ("reserved", "<i4")], align=True)
WEAK_RESULT = np.dtype([("stream", "<i4"), ("sat_id", "<i4"), ("doppler_hz", "<f8"), ("code_phase", "<i4"), ("reserved0", "<i4"),
                        ("carrier_phase", "<f8"), ("z", "<f8"), ("peak_ratio", "<f8"), ("set", "<i4"), ("reserved", "<i4")], align=True)
GYP_HYB_ALTERNATE, GYP_HYB_CODE_DOPPLER = 1, 2
WEAK_PARAMS = np.dtype([("period_ms", "<i4"), ("sync_ms", "<i4"), ("spacing", "<i8"), ("pll_bw_hz", "<f8"), ("dll_bw_hz", "<f8"),
                        ("lose_mu", "<f8"), ("reserved", "<f8")], align=True)
WEAK_MS_REC = np.dtype([("minus_re", "<f4"), ("minus_im", "<f4"), ("prompt_re", "<f4"), ("prompt_im", "<f4"), ("plus_re", "<f4"),
                        ("plus_im", "<f4"), ("pos", "<i2"), ("phase", "i1"), ("status", "i1"), ("reserved", "<i4")], align=True)
WEAK_PERIOD_REC = np.dtype([("first_ms", "<i8"), ("f", "<f8"), ("u0", "<f8"), ("c0", "<i8"), ("i", "<f8"), ("q", "<f8"), ("mu", "<f8"),
                            ("dphi", "<f8"), ("dd", "<f8"), ("bit", "<i4"), ("status", "<i4"), ("mu_mean", "<f8")], align=True)
WEAK_STATE = np.dtype([("f", "<f8"), ("f_int", "<f8"), ("u0", "<f8"), ("c0", "<i8"), ("phase", "<i4"), ("edge", "<i4"), ("status", "<i4"),
                       ("pos", "<i4"), ("n_periods", "<i4"), ("reserved", "<i4"), ("mu_mean", "<f8")], align=True)
GYP_WEAK_SYNC, GYP_WEAK_WAIT, GYP_WEAK_TRACK = 0, 1, 2
WEAK_REFINE_PARAMS = np.dtype([("span_hz", "<f8"), ("step_hz", "<f8"), ("presum_ms", "<i4"), ("reserved", "<i4")], align=True)
WEAK_REFINED = np.dtype([("stream", "<i4"), ("sat_id", "<i4"), ("doppler_hz", "<f8"), ("code_phase", "<i4"), ("edge", "<i4"),
                         ("carrier_phase", "<f8"), ("delta_hz", "<f8"), ("peak_to_mean", "<f8"), ("edge_ratio", "<f8"), ("bin", "<i4"),
                         ("status", "<i4")], align=True)
WEAK_MEASURE_PARAMS = np.dtype([("spacing", "<i8"), ("passes", "<i4"), ("reserved", "<i4")], align=True)
WEAK_MEASURED = np.dtype([("stream", "<i4"), ("sat_id", "<i4"), ("doppler_hz", "<f8"), ("carrier_phase", "<f8"), ("c0", "<i8"),
                          ("code_phase_samples", "<f8"), ("delta_chips", "<f8"), ("dd_last", "<f8"), ("cn0_dbhz", "<f8"), ("edge", "<i4"),
                          ("n_groups", "<i4"), ("status", "<i4"), ("reserved", "<i4")], align=True)
WEAK_MEASURE_FOLD = np.dtype([("e_minus", "<f8"), ("e_prompt", "<f8"), ("e_plus", "<f8"), ("wn", "<f8"), ("dd", "<f8"), ("cn0_dbhz", "<f8"),
                              ("c0", "<i8"), ("n_groups", "<i4"), ("status", "<i4")], align=True)
GYP_POWER_HIST_BINS = 2048
GYP_EXCISE_FRAME = 256
GYP_WINDOW_RECT, GYP_WINDOW_HANN = 0, 1
GYP_NOTCH_MAX_TONES = 8
GYP_BIT_ZERO, GYP_BIT_ONE, GYP_BIT_UNKNOWN = 0, 1, 2
GYP_COMM_ID_BYTES = 128
# sizeof() of every record the header declares, derived from the mirrors above (tests/test_abi_and_host.py compiles the
# header with gcc and checks sizes and offsets against them)
RECORD_SIZES = {"gyp_bit_event": BIT_EVENT.itemsize, "gyp_bits_state": BITS_STATE.itemsize, "gyp_synth_sat": SYNTH_SAT.itemsize,
                "gyp_cell_desc": CELL_DESC.itemsize, "gyp_cell": CELL.itemsize, "gyp_acq_result": ACQ_RESULT.itemsize,
                "gyp_chan_in": CHAN_IN.itemsize, "gyp_chan_out": CHAN_OUT.itemsize, "gyp_best_bin": BEST_BIN.itemsize,
                "gyp_params": PARAMS.itemsize, "gyp_track_rec": TRACK_REC.itemsize, "gyp_packing": PACKING.itemsize,
                "gyp_iq_stats": IQ_STATS.itemsize, "gyp_iq_level": IQ_LEVEL.itemsize,
                "gyp_tone_rec": TONE_REC.itemsize, "gyp_notch_tones": NOTCH_TONES.itemsize,
                "gyp_quality_sums": QUALITY_SUMS.itemsize, "gyp_quality": QUALITY.itemsize, "gyp_blanker": BLANKER.itemsize,
                "gyp_excisor": EXCISOR.itemsize, "gyp_hybrid_cell": HYBRID_CELL.itemsize, "gyp_weak_result": WEAK_RESULT.itemsize,
                "gyp_weak_params": WEAK_PARAMS.itemsize, "gyp_weak_ms_rec": WEAK_MS_REC.itemsize,
                "gyp_weak_period_rec": WEAK_PERIOD_REC.itemsize, "gyp_weak_state": WEAK_STATE.itemsize,
                "gyp_weak_refine_params": WEAK_REFINE_PARAMS.itemsize, "gyp_weak_refined": WEAK_REFINED.itemsize,
                "gyp_weak_measure_params": WEAK_MEASURE_PARAMS.itemsize, "gyp_weak_measured": WEAK_MEASURED.itemsize,
                "gyp_weak_measure_fold": WEAK_MEASURE_FOLD.itemsize}
# include/gypsum_hip.h GYP_VERSION these mirrors were written against: load() refuses any other library
GYP_VERSION = 209

EXPORTS = (
    "gyp_version gyp_create gyp_destroy gyp_last_error gyp_device_name gyp_set_stream gyp_sync gyp_wait_for gyp_timer_start "
    "gyp_timer_stop gyp_set_stream_format gyp_prn_chips gyp_prn_spectrum_lane_layout gyp_malloc gyp_free "
    "gyp_memcpy_h2d gyp_memcpy_d2h gyp_memcpy_d2h_async gyp_cell_strength gyp_correlate_cells_dev gyp_correlate_cells gyp_correlate_grid_dev "
    "gyp_correlate_grid gyp_acquire_dev gyp_params_default gyp_set_params gyp_get_params gyp_search_level_dev gyp_search_level "
    "gyp_acquire gyp_track_step_dev gyp_track_step gyp_bank_create gyp_bank_destroy gyp_bank_size gyp_bank_set_channel gyp_bank_drop_channel "
    "gyp_track_block_dev gyp_track_block gyp_bank_get_state gyp_bank_keep_profiles gyp_bank_read_profiles gyp_synth_iq_dev gyp_synth_nav_bit gyp_bank_reset_dev gyp_debug_track_profile gyp_debug_fft_bench gyp_debug_spec_read gyp_debug_dll_read gyp_debug_disc_read gyp_debug_track_timing gyp_debug_set gyp_debug_get gyp_debug_spec_redo_read gyp_debug_spec_layout gyp_debug_spec_layout_for gyp_device_locality "
    "gyp_grid_best_bins_dev gyp_grid_best_bins_refined_dev gyp_comm_unique_id gyp_comm_init gyp_comm_destroy gyp_comm_info gyp_allgather_dev gyp_host_alloc gyp_host_free gyp_widen_iq_dev "
    "gyp_bits_create gyp_bits_destroy gyp_bits_reset gyp_bits_push gyp_bits_push_block gyp_bits_drain gyp_bits_get_state "
    "gyp_ingest_open gyp_ingest_close gyp_ingest_total_ms gyp_ingest_set_scale gyp_ingest_seek gyp_ingest_next_host gyp_ingest_next_dev gyp_ingest_times "
    "gyp_resample_design gyp_resample_iq_dev gyp_ingest_open_resampled gyp_ddc_design gyp_ddc_iq_dev gyp_ingest_open_ddc "
    "gyp_packed_span gyp_unpack_iq_dev gyp_resample_packed_dev gyp_ingest_open_packed "
    "gyp_iq_stats_dev gyp_condition_iq_dev gyp_iq_level_from_stats gyp_ingest_set_level gyp_ingest_get_level gyp_ingest_calibrate "
    "gyp_iq_tones_dev gyp_notch_iq_dev gyp_tones_find gyp_tone_refine gyp_ingest_set_notches gyp_ingest_get_notches gyp_ingest_find_tones "
    "gyp_track_quality_dev gyp_track_quality gyp_quality_from_sums "
    "gyp_blank_iq_dev gyp_iq_power_hist_dev gyp_blank_from_hist gyp_ingest_set_blanker gyp_ingest_get_blanker gyp_ingest_find_pulses "
    "gyp_ingest_last_blanked "
    "gyp_excise_iq_dev gyp_iq_spectrum_hist_dev gyp_excise_from_hist gyp_ingest_set_excisor gyp_ingest_get_excisor gyp_ingest_find_excisor "
    "gyp_ingest_last_excised "
    "gyp_hybrid_stats gyp_hybrid_shift gyp_correlate_grid_hybrid_dev gyp_correlate_grid_hybrid gyp_acquire_weak_dev gyp_acquire_weak "
    "gyp_weak_params_default gyp_weak_bit_sync gyp_weak_bank_create gyp_weak_bank_destroy gyp_weak_bank_size gyp_weak_bank_set_channel "
    "gyp_weak_bank_drop_channel gyp_weak_bank_get_state gyp_weak_bank_set_state gyp_weak_track_block_dev gyp_weak_track_block "
    "gyp_weak_refine_params_default gyp_weak_refine_estimate gyp_weak_refine_dev gyp_weak_refine "
    "gyp_weak_measure_params_default gyp_weak_measure_estimate gyp_weak_measured_state gyp_weak_measure_dev gyp_weak_measure"
).split()


class GypsumHipError(RuntimeError):
    def __init__(self, code: int, message: str) -> None:
        super().__init__(f"libgypsum_hip error {code}: {message}")
        self.code = code


_lib = None


def load() -> C.CDLL:
    """dlopen the in-tree library.  There is deliberately no fallback of any kind."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m gypsum_amd.build` (hipcc --offload-arch=gfx950). "
            "gypsum_amd has no CPU or PyTorch fallback.")
    lib = C.CDLL(str(LIB_PATH))
    lib.gyp_version.restype = C.c_int
    if lib.gyp_version() != GYP_VERSION:
        raise ImportError(f"{LIB_PATH} reports ABI version {lib.gyp_version()}, this binding is written against {GYP_VERSION}: "
                          "rebuild it with `python -m gypsum_amd.build --force`")
    vp, i32, i64, u64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
    sig = {
        "gyp_version": (C.c_int, []),
        "gyp_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "gyp_destroy": (None, [vp]),
        "gyp_last_error": (C.c_char_p, [vp]),
        "gyp_device_name": (C.c_int, [vp, C.c_char_p, C.c_int]),
        "gyp_set_stream": (C.c_int, [vp, vp]),
        "gyp_sync": (C.c_int, [vp]),
        "gyp_wait_for": (C.c_int, [vp, vp]),
        "gyp_timer_start": (C.c_int, [vp]),
        "gyp_timer_stop": (C.c_int, [vp, C.POINTER(C.c_float)]),
        "gyp_set_stream_format": (C.c_int, [vp, i64, i32]),
        "gyp_prn_chips": (C.c_int, [vp]),
        "gyp_prn_spectrum_lane_layout": (C.c_int, [C.c_int, vp]),
        "gyp_malloc": (C.c_int, [vp, u64, C.POINTER(vp)]),
        "gyp_free": (C.c_int, [vp, vp]),
        "gyp_memcpy_h2d": (C.c_int, [vp, vp, vp, u64]),
        "gyp_memcpy_d2h": (C.c_int, [vp, vp, vp, u64]),
        "gyp_memcpy_d2h_async": (C.c_int, [vp, vp, vp, u64]),
        "gyp_cell_strength": (dbl, [vp, i32]),
        "gyp_correlate_cells_dev": (C.c_int, [vp, vp, i64, i32, vp, i32, i32, vp, vp]),
        "gyp_correlate_cells": (C.c_int, [vp, vp, i32, i32, vp, i32, i32, vp, vp]),
        "gyp_correlate_grid_dev": (C.c_int, [vp, vp, i32, i64, i32, vp, i32, vp, i32, i32, vp]),
        "gyp_correlate_grid": (C.c_int, [vp, vp, i32, i32, vp, i32, vp, i32, i32, vp]),
        "gyp_acquire_dev": (C.c_int, [vp, vp, i32, i64, i32, vp, i32, vp]),
        "gyp_acquire": (C.c_int, [vp, vp, i32, i32, vp, i32, vp]),
        "gyp_search_level_dev": (C.c_int, [vp, vp, i32, i64, i32, vp, i32, dbl, dbl, vp]),
        "gyp_search_level": (C.c_int, [vp, vp, i32, i32, vp, i32, dbl, dbl, vp]),
        "gyp_params_default": (None, [vp]),
        "gyp_set_params": (C.c_int, [vp, vp]),
        "gyp_get_params": (C.c_int, [vp, vp]),
        "gyp_track_step_dev": (C.c_int, [vp, vp, i64, vp, vp, i32, vp, vp]),
        "gyp_track_step": (C.c_int, [vp, vp, i32, vp, vp, i32, vp, vp]),
        "gyp_bank_create": (C.c_int, [vp, vp, i32, C.POINTER(vp)]),
        "gyp_bank_destroy": (None, [vp]),
        "gyp_bank_size": (C.c_int, [vp]),
        "gyp_bank_set_channel": (C.c_int, [vp, i32, vp]),
        "gyp_bank_drop_channel": (C.c_int, [vp, i32]),
        "gyp_track_block_dev": (C.c_int, [vp, vp, i64, i32, vp, vp]),
        "gyp_track_block": (C.c_int, [vp, vp, i32, i32, vp, vp]),
        "gyp_bank_get_state": (C.c_int, [vp, vp, vp, vp, vp]),
        "gyp_bank_keep_profiles": (C.c_int, [vp, i32]),
        "gyp_bank_read_profiles": (C.c_int, [vp, i32, vp, vp]),
        "gyp_bank_reset_dev": (C.c_int, [vp, vp]),
        "gyp_debug_track_profile": (C.c_int, [vp, C.c_int, vp]),
        "gyp_debug_fft_bench": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
        "gyp_debug_spec_read": (C.c_int, [vp, vp, i32, vp]),
        "gyp_debug_dll_read": (C.c_int, [vp, vp]),
        "gyp_debug_disc_read": (C.c_int, [vp, i32, vp]),
        "gyp_debug_track_timing": (C.c_int, [vp, C.c_int, vp]),
        "gyp_debug_spec_redo_read": (C.c_int, [vp, vp]),
        "gyp_debug_spec_layout": (C.c_int, [C.c_int32, vp]),
        "gyp_debug_spec_layout_for": (C.c_int, [C.c_int32, C.c_int32, vp]),
        "gyp_device_locality": (C.c_int, [vp, C.POINTER(i32), C.c_char_p, i32]),
        "gyp_debug_set": (C.c_int, [vp, C.c_char_p, dbl]),
        "gyp_debug_get": (C.c_int, [vp, C.c_char_p, C.POINTER(dbl)]),
        "gyp_grid_best_bins_dev": (C.c_int, [vp, vp, i32, i32, vp]),
        "gyp_grid_best_bins_refined_dev": (C.c_int, [vp, vp, i32, i64, i32, vp, i32, vp, i32, i32, vp, vp]),
        "gyp_comm_unique_id": (C.c_int, [vp]),
        "gyp_comm_init": (C.c_int, [vp, i32, i32, vp]),
        "gyp_comm_destroy": (C.c_int, [vp]),
        "gyp_comm_info": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "gyp_allgather_dev": (C.c_int, [vp, vp, vp, u64]),
        "gyp_host_alloc": (C.c_int, [vp, u64, C.POINTER(vp)]),
        "gyp_host_free": (C.c_int, [vp, vp]),
        "gyp_widen_iq_dev": (C.c_int, [vp, i32, vp, u64, C.c_float, vp]),
        "gyp_synth_iq_dev": (C.c_int, [vp, vp, i32, i64, i32, vp, i32, C.c_float, u64]),
        "gyp_synth_nav_bit": (C.c_int, [u64, i32, i32, i32, i64]),
        "gyp_bits_create": (C.c_int, [i32, C.POINTER(vp)]),
        "gyp_bits_destroy": (None, [vp]),
        "gyp_bits_reset": (C.c_int, [vp, i32]),
        "gyp_bits_push": (C.c_int, [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, C.POINTER(i32)]),
        "gyp_bits_push_block": (C.c_int, [vp, vp, i32, i32, vp, vp, vp, i32, C.POINTER(i32)]),
        "gyp_bits_drain": (C.c_int, [vp, vp, i32, C.POINTER(i32)]),
        "gyp_bits_get_state": (C.c_int, [vp, i32, vp]),
        "gyp_ingest_open": (C.c_int, [vp, C.c_char_p, i32, i64, i32, i32, i32, C.POINTER(vp)]),
        "gyp_ingest_close": (None, [vp]),
        "gyp_ingest_total_ms": (i64, [vp]),
        "gyp_ingest_set_scale": (C.c_int, [vp, C.c_float]),
        "gyp_ingest_seek": (C.c_int, [vp, i64]),
        "gyp_ingest_next_host": (C.c_int, [vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(i32)]),
        "gyp_ingest_next_dev": (C.c_int, [vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(i32)]),
        "gyp_ingest_times": (C.c_int, [vp, i64, i32, vp, vp]),
        "gyp_resample_design": (C.c_int, [i64, i64, i32, vp, C.POINTER(i32)]),
        "gyp_resample_iq_dev": (C.c_int, [vp, i32, vp, i32, i64, i64, i64, C.c_float, i64, i32, i64, i32, i64, vp]),
        "gyp_ingest_open_resampled": (C.c_int, [vp, C.c_char_p, i32, i64, i32, i32, i32, C.POINTER(vp)]),
        "gyp_ddc_design": (C.c_int, [i64, i64, i64, i32, vp, C.POINTER(i32), C.POINTER(i32)]),
        "gyp_ddc_iq_dev": (C.c_int, [vp, i32, vp, i32, i64, i64, i64, C.c_float, i64, i64, i32, i64, i32, i64, vp]),
        "gyp_ingest_open_ddc": (C.c_int, [vp, C.c_char_p, i32, i64, i64, i32, i32, i32, C.POINTER(vp)]),
        "gyp_packed_span": (C.c_int, [vp, i32, i64, i64, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i32),
                                      C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]),
        "gyp_unpack_iq_dev": (C.c_int, [vp, vp, vp, i32, i64, i32, i64, C.c_float, i64, vp]),
        "gyp_resample_packed_dev": (C.c_int, [vp, vp, vp, i32, i64, i32, i64, i64, C.c_float, i64, i64, i32, i64, i32, i64, vp]),
        "gyp_ingest_open_packed": (C.c_int, [vp, C.c_char_p, vp, i64, i64, i32, i32, i32, C.POINTER(vp)]),
        "gyp_iq_stats_dev": (C.c_int, [vp, vp, i32, i64, i32, i32, C.c_float, vp]),
        "gyp_condition_iq_dev": (C.c_int, [vp, vp, vp, i32, i64, i64, vp]),
        "gyp_iq_level_from_stats": (C.c_int, [vp, i32, i32, i32, dbl, vp, vp]),
        "gyp_ingest_set_level": (C.c_int, [vp, vp]),
        "gyp_ingest_get_level": (C.c_int, [vp, vp, C.POINTER(i32)]),
        "gyp_ingest_calibrate": (C.c_int, [vp, i64, i32, i32, dbl, C.c_float, vp, vp]),
        "gyp_iq_tones_dev": (C.c_int, [vp, vp, i32, i64, i64, i32, i32, i64, vp, i32, i32, vp]),
        "gyp_notch_iq_dev": (C.c_int, [vp, vp, vp, i32, i64, i64, i32, i32, i64, vp]),
        "gyp_tones_find": (C.c_int, [vp, i32, dbl, dbl, i32, i32, vp]),
        "gyp_tone_refine": (C.c_int, [vp, i32, dbl, C.POINTER(dbl)]),
        "gyp_ingest_set_notches": (C.c_int, [vp, vp, i32]),
        "gyp_ingest_get_notches": (C.c_int, [vp, vp, C.POINTER(i32)]),
        "gyp_ingest_find_tones": (C.c_int, [vp, i64, i32, dbl, i32, i32, vp, vp, C.POINTER(i32)]),
        "gyp_track_quality_dev": (C.c_int, [vp, vp, i32, i64, i32, i32, vp, vp]),
        "gyp_track_quality": (C.c_int, [vp, vp, i32, i64, i32, i32, vp, vp]),
        "gyp_quality_from_sums": (C.c_int, [vp, i32, vp]),
        "gyp_blank_iq_dev": (C.c_int, [vp, vp, vp, i32, i64, i32, i32, vp, vp]),
        "gyp_iq_power_hist_dev": (C.c_int, [vp, vp, i32, i64, i64, vp, vp]),
        "gyp_blank_from_hist": (C.c_int, [vp, C.c_float, C.c_float, dbl, i32, vp, vp]),
        "gyp_ingest_set_blanker": (C.c_int, [vp, vp]),
        "gyp_ingest_get_blanker": (C.c_int, [vp, vp, C.POINTER(i32)]),
        "gyp_ingest_find_pulses": (C.c_int, [vp, i64, i32, i32, dbl, i32, i32, vp, vp]),
        "gyp_ingest_last_blanked": (C.c_int, [vp, vp, i32, C.POINTER(i32)]),
        "gyp_excise_iq_dev": (C.c_int, [vp, vp, vp, i32, i64, i32, i32, vp, vp, vp]),
        "gyp_iq_spectrum_hist_dev": (C.c_int, [vp, vp, i32, i64, i32, i32, vp]),
        "gyp_excise_from_hist": (C.c_int, [vp, dbl, i32, vp, vp]),
        "gyp_ingest_set_excisor": (C.c_int, [vp, vp]),
        "gyp_ingest_get_excisor": (C.c_int, [vp, vp, C.POINTER(i32)]),
        "gyp_ingest_find_excisor": (C.c_int, [vp, i64, i32, dbl, i32, i32, vp, vp]),
        "gyp_ingest_last_excised": (C.c_int, [vp, vp, i32, C.POINTER(i32)]),
        "gyp_hybrid_stats": (C.c_int, [vp, C.POINTER(dbl), C.POINTER(dbl)]),
        "gyp_hybrid_shift": (i32, [i32, i32, i32, dbl, i32]),
        "gyp_correlate_grid_hybrid_dev": (C.c_int, [vp, vp, i32, i64, i32, i32, i32, vp, i32, vp, i32, vp]),
        "gyp_correlate_grid_hybrid": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, i32, vp, i32, vp]),
        "gyp_acquire_weak_dev": (C.c_int, [vp, vp, i32, i64, i32, i32, i32, dbl, dbl, dbl, vp, i32, vp]),
        "gyp_acquire_weak": (C.c_int, [vp, vp, i32, i32, i32, i32, dbl, dbl, dbl, vp, i32, vp]),
        "gyp_weak_params_default": (None, [vp]),
        "gyp_weak_bit_sync": (C.c_int, [vp, i32, i64, vp, vp]),
        "gyp_weak_bank_create": (C.c_int, [vp, vp, i32, vp, i64, C.POINTER(vp)]),
        "gyp_weak_bank_destroy": (None, [vp]),
        "gyp_weak_bank_size": (C.c_int, [vp]),
        "gyp_weak_bank_set_channel": (C.c_int, [vp, i32, vp]),
        "gyp_weak_bank_drop_channel": (C.c_int, [vp, i32]),
        "gyp_weak_bank_get_state": (C.c_int, [vp, vp, C.POINTER(i64)]),
        "gyp_weak_bank_set_state": (C.c_int, [vp, i32, vp]),
        "gyp_weak_track_block_dev": (C.c_int, [vp, vp, i64, i64, i32, vp, vp, vp]),
        "gyp_weak_track_block": (C.c_int, [vp, vp, i32, i64, i32, vp, vp, vp]),
        "gyp_weak_refine_params_default": (None, [vp]),
        "gyp_weak_refine_estimate": (C.c_int, [vp, i32, i64, vp, vp]),
        "gyp_weak_refine_dev": (C.c_int, [vp, vp, i32, i64, i64, i32, vp, i32, vp, vp, vp]),
        "gyp_weak_refine": (C.c_int, [vp, vp, i32, i64, i32, vp, i32, vp, vp, vp]),
        "gyp_weak_measure_params_default": (None, [vp]),
        "gyp_weak_measure_estimate": (C.c_int, [vp, vp, i32, i64, i32, i64, i64, vp]),
        "gyp_weak_measured_state": (C.c_int, [vp, i64, i32, i32, vp]),
        "gyp_weak_measure_dev": (C.c_int, [vp, vp, i32, i64, i64, i32, vp, i32, vp, vp, vp, vp, vp]),
        "gyp_weak_measure": (C.c_int, [vp, vp, i32, i64, i32, vp, i32, vp, vp, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)   # AttributeError here == the library does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def ptr(a) -> C.c_void_p:
    """Raw pointer of a C-contiguous numpy array (or None)."""
    if a is None:
        return C.c_void_p(None)
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("array must be C-contiguous")
    return C.c_void_p(a.ctypes.data)
