"""Narrowband and swept interference in a recording: the excisor of libgypsum_hip (include/gypsum_hip.h, "excisor").

A carrier with FM or AM on it, a narrowband digital signal, a drifting spur, a slow swept jammer, more tones than a notch list
holds: continuous, so the blanker cannot touch it, and no pure tone, so a notch cannot follow it.  The device takes half-overlapped
256-point transforms of every millisecond, a histogram of the bins' power, the host puts a threshold a factor above its median, and
the ingest zeroes every bin that reaches it -- and `guard` bins on either side -- and subtracts what those bins held, behind the
blanker and in front of notches and level:

    ing = IqFileIngest(path, fs, np.int8, engine=engine)
    excisor, measured = ing.find_excisor(first_ms=0, n_ms=10)   # threshold^2 = 16 x the median bin power; installed
    level, _ = ing.calibrate(first_ms=0, n_ms=100)              # measures the excised output
    first_ms, n_ms, dev = ing.next_device_block()               # producer -> blanker -> excisor -> notches -> level, in HBM
    counts = ing.last_excised()                                 # excised (frame, bin) cells per millisecond of that block

An excisor known beforehand is installed with `ing.set_excisor(Excisor(threshold=40.0, guard=1))`; `engine.spectrum_hist(iq, n)`,
`excisor_from_hist(hist, ...)` and `engine.excise_iq(iq, samples_per_ms, excisors)` are the steps on host arrays.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import _lib, _records

# one per stream: gyp_excisor, 16 bytes
EXCISOR_DTYPE = _lib.EXCISOR
HIST_BINS = _lib.GYP_POWER_HIST_BINS
FRAME = _lib.GYP_EXCISE_FRAME
HOP = FRAME // 2
MAX_GUARD = 8
MAX_SAMPLES_PER_MS = 65536


def n_frames(samples_per_ms: int) -> int:
    """Frames per millisecond: ceil((n + 128) / 128)."""
    return (int(samples_per_ms) + HOP - 1) // HOP + 1


@dataclass(frozen=True)
class Excisor(_records.Record):
    """A bin of a 256-point frame whose |X| reaches `threshold` is excised, with `guard` bins on either side (gyp_excisor)."""
    threshold: float = 1.0
    guard: int = 1
    DTYPE, MEASURED = EXCISOR_DTYPE, ("median", "threshold")


def excisor_records(excisors, n_streams: int = None) -> np.ndarray:
    """One gyp_excisor record per stream from `excisors`: records already, one Excisor (for one stream, or for each of n_streams
    streams) or a sequence of them."""
    return _records.records(excisors, Excisor, n_streams)


def check_excisor(excisor: Excisor) -> None:
    """ValueError unless the excisor is one the device takes (positive finite float32 threshold, guard 0..8)."""
    rec = excisor.record()[0]
    if not (float(rec["threshold"]) > 0.0 and math.isfinite(float(rec["threshold"]))):
        raise ValueError("the threshold must be positive and finite in float32")
    if int(excisor.guard) != excisor.guard or not 0 <= int(excisor.guard) <= MAX_GUARD:
        raise ValueError(f"the guard must be a whole number in 0 .. {MAX_GUARD}")


def excisor_from_hist(hist: np.ndarray, threshold_over_median: float = 16.0, guard: int = 1) -> Tuple[Excisor, dict]:
    """The excisor whose threshold is sqrt(threshold_over_median x the median bin power) of one stream's histogram
    (gyp_excise_from_hist: host only, no GPU).  Returns (excisor, measured) with measured = {"median", "threshold"} in float64."""
    h = _records.one_hist(hist)
    return _records.derived(Excisor, lambda lib, rec, measured: lib.gyp_excise_from_hist(
        _lib.ptr(h), float(threshold_over_median), int(guard), rec, measured))


def measured_dict(measured2: np.ndarray) -> dict:
    return _records.measured_dict(Excisor, measured2)
