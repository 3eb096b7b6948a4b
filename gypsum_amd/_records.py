"""Behind level.IqLevel, blanker.Blanker and excisor.Excisor: dataclasses whose fields are named as their numpy `DTYPE`'s, with
the names `MEASURED` of what a measurement reports beside the record.  Their `record()` / `from_record()`, and the modules'
`*_records`, `*_from_*` and `measured_dict`."""
from __future__ import annotations

import dataclasses

import numpy as np

from . import _lib


class Record:
    def record(self) -> np.ndarray:
        rec = np.zeros(1, dtype=self.DTYPE)
        with np.errstate(over="ignore"):                    # (a value beyond float32 becomes inf, which the stage's check refuses)
            for f in dataclasses.fields(self):
                rec[f.name] = type(f.default)(getattr(self, f.name))
        return rec

    @classmethod
    def from_record(cls, rec):
        r = np.asarray(rec, dtype=cls.DTYPE).reshape(-1)[0]
        return cls(*(type(f.default)(r[f.name]) for f in dataclasses.fields(cls)))


def records(values, cls, n_streams: int = None) -> np.ndarray:
    """One record per stream from `values`: records already, one `cls` (for one stream, or for each of n_streams streams) or a
    sequence of them."""
    if isinstance(values, np.ndarray) and values.dtype == cls.DTYPE:
        return np.ascontiguousarray(values).reshape(-1)
    if isinstance(values, cls):
        values = [values] * (1 if n_streams is None else max(1, int(n_streams)))
    return np.concatenate([v.record() for v in values])


def measured_dict(cls, measured: np.ndarray) -> dict:
    return {name: float(value) for name, value in zip(cls.MEASURED, measured)}


def derived(cls, call):
    """(the `cls` that the host-only call(lib, record pointer, measured pointer) derives, what it measured as a dict)."""
    lib = _lib.load()
    rec, measured = np.zeros(1, dtype=cls.DTYPE), np.zeros(len(cls.MEASURED))
    rc = call(lib, _lib.ptr(rec), _lib.ptr(measured))
    if rc != 0:
        raise _lib.GypsumHipError(rc, (lib.gyp_last_error(None) or b"").decode())
    return cls.from_record(rec), measured_dict(cls, measured)


def one_hist(hist) -> np.ndarray:
    """One stream's histogram as the library takes it."""
    h = np.ascontiguousarray(hist, dtype=np.uint32).reshape(-1)
    if len(h) != _lib.GYP_POWER_HIST_BINS:
        raise ValueError(f"a histogram has {_lib.GYP_POWER_HIST_BINS} bins")
    return h


@dataclasses.dataclass
class WeakParams(Record):
    """gyp_weak_params, with the library's defaults (gyp_weak_params_default): the 20-ms period, the correlator spacing in 2^-40
    chips, the open-loop span before the bit edge is picked, the loop bandwidths and the NBP / WBP mean below which a channel is lost."""
    DTYPE = _lib.WEAK_PARAMS
    period_ms: int = 20
    sync_ms: int = 400
    spacing: int = 1 << 39
    pll_bw_hz: float = 8.0
    dll_bw_hz: float = 1.0
    lose_mu: float = 2.5
    reserved: float = 0.0


@dataclasses.dataclass
class WeakRefineParams(Record):
    """gyp_weak_refine_params, with the library's defaults (gyp_weak_refine_params_default): the half width and the step of the
    residual-Doppler scan in Hz and the milliseconds of prompts summed before squaring."""
    DTYPE = _lib.WEAK_REFINE_PARAMS
    span_hz: float = 20.0
    step_hz: float = 0.5
    presum_ms: int = 4
    reserved: int = 0


@dataclasses.dataclass
class WeakMeasureParams(Record):
    """gyp_weak_measure_params, with the library's defaults (gyp_weak_measure_params_default): the early / late spacing in 2^-40 chips
    and the number of passes, each of which corrects the code phase once."""
    DTYPE = _lib.WEAK_MEASURE_PARAMS
    spacing: int = 1 << 39
    passes: int = 2
    reserved: int = 0
