"""Pulsed (wideband) interference in a recording: the blanker of libgypsum_hip (include/gypsum_hip.h, "blanker").

Radar, DME-like bursts, ignition noise, a neighbouring transmitter keying up, ADC saturation bursts: a pulse is broadband, so a
notch does nothing to it, and brief, so an RMS-based level is wrong in both directions.  The device takes a histogram of the power
about the recording's centre, the host puts a threshold a factor above its median, and the ingest replaces every sample that
reaches it -- and `guard` neighbours on either side, within the same millisecond -- by the centre, in front of notches and level:

    ing = IqFileIngest(path, fs_out, np.uint8, engine=engine, resample_from_hz=2_048_000)
    blanker, measured = ing.find_pulses(first_ms=0, n_ms=10)  # threshold^2 = 16 x the median power; installed
    tones = ing.find_tones(first_ms=0, n_ms=10)               # searches the BLANKED output
    level, _ = ing.calibrate(first_ms=0, n_ms=100)            # measures the blanked and notched output
    first_ms, n_ms, dev = ing.next_device_block()             # producer -> blanker -> notches -> level, in HBM
    counts = ing.last_blanked()                               # blanked samples per millisecond of that block

A blanker known beforehand is installed with `ing.set_blanker(Blanker(0.0, 0.0, 4.2, guard=4))`; `engine.power_hist(iq, centres)`,
`blanker_from_hist(hist, ...)` and `engine.blank_iq(iq, samples_per_ms, blankers)` are the steps on host arrays.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import _lib, _records

# one per stream: gyp_blanker, 16 bytes
BLANKER_DTYPE = _lib.BLANKER
HIST_BINS = _lib.GYP_POWER_HIST_BINS
MAX_GUARD = 64
MAX_SAMPLES_PER_MS = 65536


@dataclass(frozen=True)
class Blanker(_records.Record):
    """A sample whose |x - centre| reaches `threshold` is replaced by the centre, with `guard` samples on either side (gyp_blanker)."""
    center_re: float = 0.0
    center_im: float = 0.0
    threshold: float = 1.0
    guard: int = 0
    DTYPE, MEASURED = BLANKER_DTYPE, ("median", "threshold")


def blanker_records(blankers, n_streams: int = None) -> np.ndarray:
    """One gyp_blanker record per stream from `blankers`: records already, one Blanker (for one stream, or for each of n_streams
    streams) or a sequence of them."""
    return _records.records(blankers, Blanker, n_streams)


def check_blanker(blanker: Blanker) -> None:
    """ValueError unless the blanker is one the device takes (finite centre, positive finite float32 threshold, guard 0..64)."""
    rec = blanker.record()[0]
    if not (math.isfinite(float(rec["center_re"])) and math.isfinite(float(rec["center_im"]))):
        raise ValueError("the centre must be finite")
    if not (float(rec["threshold"]) > 0.0 and math.isfinite(float(rec["threshold"]))):
        raise ValueError("the threshold must be positive and finite in float32")
    if int(blanker.guard) != blanker.guard or not 0 <= int(blanker.guard) <= MAX_GUARD:
        raise ValueError(f"the guard must be a whole number in 0 .. {MAX_GUARD}")


def bin_edges() -> np.ndarray:
    """The 2049 lower edges of the histogram's bins as float64: edge k is the float32 whose bits are k << 20 (edge 2040 is +inf,
    the ones above are NaN: those bins hold the non-finite powers)."""
    with np.errstate(invalid="ignore"):
        return (np.arange(HIST_BINS + 1, dtype=np.uint32) << np.uint32(20)).view(np.float32).astype(np.float64)


def blanker_from_hist(hist: np.ndarray, center=(0.0, 0.0), threshold_over_median: float = 16.0, guard: int = 4) -> Tuple[Blanker, dict]:
    """The blanker whose threshold is sqrt(threshold_over_median x the median power) of one stream's histogram
    (gyp_blank_from_hist: host only, no GPU).  Returns (blanker, measured) with measured = {"median", "threshold"} in float64."""
    h = _records.one_hist(hist)
    return _records.derived(Blanker, lambda lib, rec, measured: lib.gyp_blank_from_hist(
        _lib.ptr(h), C.c_float(center[0]), C.c_float(center[1]), float(threshold_over_median), int(guard), rec, measured))


def measured_dict(measured2: np.ndarray) -> dict:
    return _records.measured_dict(Blanker, measured2)
