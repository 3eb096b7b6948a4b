"""Narrowband (CW) interference in a recording: the notches of libgypsum_hip (include/gypsum_hip.h, "notch").

A CW spur inside the band -- a harmonic of an RTL-SDR's 28.8 MHz reference, a USB or clock spur, a jammer -- far above the noise
jams every Doppler bin: acquisition strengths collapse towards the noise-only values and the Costas loops pull towards the
interferer.  The device measures complex amplitudes of tones per block (a brute-force spectrum scan, frequency refinement), the
host picks the tones out of the spectrum, and the ingest removes them from every block, between whatever produced it and the level:

    ing = IqFileIngest(path, fs_out, np.uint8, engine=engine, resample_from_hz=2_048_000)
    tones = ing.find_tones(first_ms=0, n_ms=10)               # [(Hz, dB over the spectrum's median), ...]; installed
    level, measured = ing.calibrate(first_ms=0, n_ms=100)     # measures the NOTCHED output
    first_ms, n_ms, dev = ing.next_device_block()             # producer -> notches -> level, in HBM

Tones known beforehand are installed with `ing.set_notches([217_300])`; `engine.iq_tones(iq, fs, freqs, block_samples)`,
`find_tones(power, ...)`, `refine(records, block_seconds)` and `engine.notch_iq(iq, fs, samples_per_ms, tones)` are the steps on
host arrays.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from . import _lib

# one per (stream, block, frequency): gyp_tone_rec, 16 bytes
TONE_DTYPE = _lib.TONE_REC
# one per stream: gyp_notch_tones, 72 bytes
NOTCH_DTYPE = _lib.NOTCH_TONES
WINDOW_RECT, WINDOW_HANN = _lib.GYP_WINDOW_RECT, _lib.GYP_WINDOW_HANN
MAX_TONES = _lib.GYP_NOTCH_MAX_TONES
MIN_SEPARATION_HZ = 4000


def notch_records(tones, n_streams: int = None) -> np.ndarray:
    """One gyp_notch_tones record per stream from `tones`: records already, one list of Hz (for one stream, or for each of n_streams
    streams) or one list per stream."""
    if isinstance(tones, np.ndarray) and tones.dtype == NOTCH_DTYPE:
        return np.ascontiguousarray(tones).reshape(-1)
    lists = list(tones)
    if not lists or not isinstance(lists[0], (list, tuple, np.ndarray)):
        lists = [lists] * (1 if n_streams is None else int(n_streams))
    rec = np.zeros(len(lists), dtype=NOTCH_DTYPE)
    for s, freqs in enumerate(lists):
        if len(freqs) > MAX_TONES:
            raise ValueError(f"stream {s}: {len(freqs)} tones (at most {MAX_TONES})")
        rec["count"][s] = len(freqs)
        rec["freq_hz"][s, :len(freqs)] = [int(f) for f in freqs]
    return rec


def _host_check(rc: int) -> int:
    if rc < 0:
        raise _lib.GypsumHipError(rc, (_lib.load().gyp_last_error(None) or b"").decode())
    return rc


def find_tones(power: np.ndarray, freq_step_hz: float, threshold_over_median: float, min_separation_bins: int,
               max_tones: int = MAX_TONES) -> List[int]:
    """The bins of the local maxima of a power spectrum that reach threshold_over_median times its median, strongest first (of equal
    powers and of equal neighbours the lowest bin), no two closer than min_separation_bins (gyp_tones_find: host only, no GPU)."""
    p = np.ascontiguousarray(power, dtype=np.float64).reshape(-1)
    bins = np.zeros(max(1, int(max_tones)), dtype=np.int32)
    n = _host_check(_lib.load().gyp_tones_find(_lib.ptr(p), len(p), float(freq_step_hz), float(threshold_over_median),
                                               int(min_separation_bins), int(max_tones), _lib.ptr(bins)))
    return [int(b) for b in bins[:n]]


def refine(records: np.ndarray, block_seconds: float) -> float:
    """Hz between a tone and the frequency its consecutive per-block records were measured at: the phase slope
    arg(sum_b A[b+1] conj(A[b])) / (2 pi block_seconds), valid for |delta| < 1 / (2 block_seconds) (gyp_tone_refine: host only)."""
    import ctypes as C
    r = np.ascontiguousarray(records, dtype=TONE_DTYPE).reshape(-1)
    delta = C.c_double()
    _host_check(_lib.load().gyp_tone_refine(_lib.ptr(r), len(r), float(block_seconds), C.byref(delta)))
    return float(delta.value)


def as_complex(records: np.ndarray) -> np.ndarray:
    """complex128 amplitudes of gyp_tone_rec records, same shape."""
    r = np.asarray(records)
    return r["re"] + 1j * r["im"]


def check_tones(freqs_hz: Sequence[int], fs_hz: int) -> None:
    """ValueError unless the list is one the notch takes at fs_hz (at most 8 tones, |f| < fs / 2, pairwise 4000 Hz apart)."""
    f = [int(x) for x in freqs_hz]
    if len(f) > MAX_TONES:
        raise ValueError(f"{len(f)} tones (at most {MAX_TONES})")
    if any(2 * abs(x) >= int(fs_hz) for x in f):
        raise ValueError("every tone must satisfy |f| < fs / 2")
    if any(abs(a - b) < MIN_SEPARATION_HZ for i, a in enumerate(f) for b in f[:i]):
        raise ValueError(f"tones must be at least {MIN_SEPARATION_HZ} Hz apart")
