"""DC offset and amplitude of a recording: the signal conditioning of libgypsum_hip (include/gypsum_hip.h, "level").

An offset-binary recording (RTL-SDR uint8, zero at 128) carries a DC term far above the noise and cannot be acquired as it is, and
the tracking loops' fixed thresholds assume GNU-Radio-like amplitudes.  The device measures per-millisecond statistics (sums, peak,
clipped components: also a level, saturation and interference monitor by themselves), the host derives one level from them, and
the ingest applies it to every block behind whatever produced it:

    ing = IqFileIngest(path, fs_out, np.uint8, engine=engine, resample_from_hz=2_048_000)
    level, measured = ing.calibrate(first_ms=0, n_ms=100)     # measures the first 100 ms, installs the level
    first_ms, n_ms, dev = ing.next_device_block()             # (x - dc) * gain, in HBM

A level known beforehand is installed with `ing.set_level(IqLevel(128.0, 128.0, 1 / 100))`; `engine.iq_stats(iq, samples_per_ms)`,
`level_from_stats(stats, samples_per_ms, target_rms)` and `engine.condition_iq(iq, level)` are the three steps on host arrays.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import _lib, _records

# one per (stream, millisecond): gyp_iq_stats, 32 bytes
STATS_DTYPE = _lib.IQ_STATS
LEVEL_DTYPE = _lib.IQ_LEVEL


def default_target_rms(samples_per_ms: int) -> float:
    """sqrt(2 / N): noise of that RMS per complex sample leaves the one-millisecond prompt correlation a variance of 1 per
    component -- inside lock_i_variance_max = 2 (tracker.py:170-186), where gypsum_amd.synth.lock_regime_scene puts its scenes.
    A recording is noise to within a fraction of a dB, so this is the level at which the loops' fixed thresholds can be met."""
    return float(np.sqrt(2.0 / int(samples_per_ms)))


@dataclass(frozen=True)
class IqLevel(_records.Record):
    """y = (x - (dc_re + 1j * dc_im)) * gain, in float32 (gyp_iq_level)."""
    dc_re: float = 0.0
    dc_im: float = 0.0
    gain: float = 1.0
    DTYPE, MEASURED = LEVEL_DTYPE, ("mean_re", "mean_im", "rms", "clipped")


def level_records(levels) -> np.ndarray:
    """One gyp_iq_level record per entry of `levels` (an IqLevel, a sequence of them, or records already)."""
    return _records.records(levels, IqLevel)


def level_from_stats(stats: np.ndarray, samples_per_ms: int, target_rms: float, remove_dc: bool = True) -> Tuple[IqLevel, dict]:
    """The level that removes the mean (remove_dc) and brings the RMS of |x| per complex sample to target_rms, from the
    per-millisecond records of one stream (gyp_iq_level_from_stats: host only, no GPU).  Returns (level, measured) with
    measured = {"mean_re", "mean_im", "rms", "clipped"}: the mean, the RMS about the removed offset, the share of clipped components."""
    st = np.ascontiguousarray(stats, dtype=STATS_DTYPE).reshape(-1)
    return _records.derived(IqLevel, lambda lib, rec, measured: lib.gyp_iq_level_from_stats(
        _lib.ptr(st), len(st), int(samples_per_ms), int(bool(remove_dc)), float(target_rms), rec, measured))


def measured_dict(measured4: np.ndarray) -> dict:
    return _records.measured_dict(IqLevel, measured4)
