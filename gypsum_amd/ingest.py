"""IQ recording ingest (`gypsum/antenna_sample_provider.py:79-136`, `radio_input.py:22-44`).

`IqFileIngest` wraps the native reader of libgypsum_hip (`gyp_ingest_*`): a reader thread fills a ring of (pinned)
host buffers with whole blocks of milliseconds; with an engine, `next_device_block()` returns the block already
uploaded (one block ahead, on a copy stream) as complex64 in HBM, integer recordings being widened on the device.
Without an engine it is a host-only block reader, which `AntennaSampleProviderBackedByFile(block_ms=...)` uses to
serve the reference's one-millisecond chunks without a file open per millisecond.

With `resample_from_hz` the recording is at that rate (any whole kHz within a factor 2 of the engine's) and the device blocks
come out resampled to the engine's stream format (`gyp_ingest_open_resampled`, `gypsum_amd.resample`); `n` and `fs` are then
the output rate and there are no host blocks.  With `if_hz` as well the recording holds one real word per sample at an
intermediate frequency of `if_hz` Hz and is down-converted to complex baseband on the device (`gyp_ingest_open_ddc`).

With `packing` (gypsum_amd.packing) the recording holds 1-, 2- or 4-bit words packed into bytes, read as they are and unpacked on
the device (`gyp_ingest_open_packed`): I,Q at the engine's rate (`resample_from_hz` None or equal to it) are only unpacked, I,Q at
another rate are resampled, and a real packing (with `if_hz`) is down-converted.  The word type is then the packing's, so
`sample_component_data_type` must be left out.

`set_level` / `calibrate` (gypsum_amd.level) remove a DC offset and normalise the amplitude of every device block, whatever
produced it: an RTL-SDR uint8 recording needs no rewrite on the host.

`set_notches` / `find_tones` (gypsum_amd.notch) remove narrowband (CW) interference from every device block, between whatever
produced it and the level: `calibrate` then measures the notched output.

`set_blanker` / `find_pulses` (gypsum_amd.blanker) blank pulsed (wideband) interference in every device block, in front of the
notches: `find_tones` and `calibrate` then measure the blanked output, and `last_blanked` counts what each block lost.
`set_excisor` / `find_excisor` (gypsum_amd.excisor) excise narrowband and swept interference in every device block, behind the
blanker and in front of the notches; `last_excised` counts the (frame, bin) cells each block lost.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Optional, Tuple

import numpy as np

from . import _lib, _records
from .blanker import Blanker
from .excisor import Excisor
from .level import IqLevel, default_target_rms

_FORMATS = {np.dtype(np.float32): _lib.GYP_FMT_F32, np.dtype(np.int8): _lib.GYP_FMT_I8,
            np.dtype(np.int16): _lib.GYP_FMT_I16, np.dtype(np.uint8): _lib.GYP_FMT_U8}


class IqFileIngest:
    def __init__(self, path, samples_per_second: int, sample_component_data_type=None, block_ms: int = 100,
                 depth: int = 4, engine=None, resample_from_hz: Optional[int] = None, taps: Optional[int] = None,
                 if_hz: Optional[int] = None, packing=None) -> None:
        self.packing = packing
        if packing is None:
            self.dtype = np.dtype(np.float32 if sample_component_data_type is None else sample_component_data_type)
            if self.dtype not in _FORMATS:
                raise ValueError(f"unsupported sample component type {self.dtype} (float32, int8, int16, uint8)")
        else:
            if sample_component_data_type is not None:
                raise ValueError("a packed recording's words are given by its packing: leave sample_component_data_type out")
            if engine is None:
                raise ValueError("packed recordings are unpacked on the device: pass an engine")
            self.dtype = None
        self._lib = _lib.load()
        self.engine = engine
        self.path = Path(path)
        self.fs = int(samples_per_second)
        self.n = self.fs // 1000
        self.block_ms = int(block_ms)
        self._h = C.c_void_p()
        self.resample_from_hz = None if resample_from_hz is None else int(resample_from_hz)
        self.if_hz = None if if_hz is None else int(if_hz)
        if packing is not None:
            self._open_packed(taps, depth)
            return
        ctx = engine.ctx if engine is not None else None
        if self.if_hz is not None and self.resample_from_hz is None:
            raise ValueError("if_hz needs resample_from_hz (the real recording's sample rate)")
        if self.resample_from_hz is not None:
            if engine is None:
                raise ValueError("resampling runs on the device: pass an engine")
            self._check_output_rate()
            if self.if_hz is not None:   # taps None: the down-converter's automatic choice
                rc = self._lib.gyp_ingest_open_ddc(ctx, str(self.path).encode(), _FORMATS[self.dtype], self.resample_from_hz, self.if_hz,
                                                   int(taps or 0), self.block_ms, int(depth), C.byref(self._h))
            else:
                rc = self._lib.gyp_ingest_open_resampled(ctx, str(self.path).encode(), _FORMATS[self.dtype], self.resample_from_hz,
                                                         32 if taps is None else int(taps), self.block_ms, int(depth), C.byref(self._h))
        else:
            rc = self._lib.gyp_ingest_open(ctx, str(self.path).encode(), _FORMATS[self.dtype], self.fs, self.n, self.block_ms,
                                           int(depth), C.byref(self._h))
        self._check(rc)

    def _check_output_rate(self) -> None:
        if self.engine.fs is not None and self.engine.fs != self.fs:
            raise ValueError(f"samples_per_second ({self.fs}) is the output rate and must be the engine's stream format ({self.engine.fs})")

    def _open_packed(self, taps, depth) -> None:
        self._check_output_rate()
        if self.resample_from_hz is None:
            self.resample_from_hz = self.fs
        if self.packing.real and self.if_hz is None:
            raise ValueError("a real packing needs if_hz (the recording's intermediate frequency)")
        if not self.packing.real and self.if_hz is not None:
            raise ValueError("if_hz is for real packings (an I,Q packing has no intermediate frequency)")
        self._record = self.packing.record()
        rc = self._lib.gyp_ingest_open_packed(self.engine.ctx, str(self.path).encode(), _lib.ptr(self._record), self.resample_from_hz,
                                              int(self.if_hz or 0), int(taps or 0), self.block_ms, int(depth), C.byref(self._h))
        self._check(rc)

    def _check(self, rc: int) -> None:
        if rc != 0:
            ctx = self.engine.ctx if self.engine is not None else None
            raise _lib.GypsumHipError(rc, (self._lib.gyp_last_error(ctx) or b"").decode())

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.gyp_ingest_close(self._h)
            self._h = C.c_void_p()

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass

    @property
    def total_ms(self) -> int:
        """Milliseconds the reference's provider delivers before NoMoreSamplesError (of the input file, when resampling)."""
        return int(self._lib.gyp_ingest_total_ms(self._h))

    def set_scale(self, scale: float) -> None:
        """Integer recordings: device samples = word * scale (default 1 = the reference's raw values)."""
        self._check(self._lib.gyp_ingest_set_scale(self._h, float(scale)))

    # What the record-valued stages (level, blanker, excisor) do alike: `cls` is IqLevel, Blanker or Excisor, `fn` the entry point
    def _set_record(self, fn, value) -> None:
        rec = None if value is None else value.record()
        self._check(fn(self._h, _lib.ptr(rec)))

    def _get_record(self, fn, cls):
        rec, on = np.zeros(1, dtype=cls.DTYPE), C.c_int32()
        self._check(fn(self._h, _lib.ptr(rec), C.byref(on)))
        return cls.from_record(rec) if on.value else None

    def _find_record(self, fn, cls, first_ms, n_ms, *args):
        rec, measured = np.zeros(1, dtype=cls.DTYPE), np.zeros(len(cls.MEASURED))
        self._check(fn(self._h, int(first_ms), int(n_ms), *args, _lib.ptr(rec), _lib.ptr(measured)))
        return cls.from_record(rec), _records.measured_dict(cls, measured)

    def _last_counts(self, fn) -> np.ndarray:
        counts, n_ms = np.zeros(self.block_ms, dtype=np.int32), C.c_int32()
        self._check(fn(self._h, _lib.ptr(counts), len(counts), C.byref(n_ms)))
        return counts[:n_ms.value]

    def set_level(self, level) -> None:
        """A gypsum_amd.level.IqLevel every device block is conditioned with from the next block handed out on: (x - dc) * gain behind
        whatever produced the block, x = word * scale as without a level (gyp_ingest_set_level).  None switches it off."""
        self._set_record(self._lib.gyp_ingest_set_level, level)

    @property
    def level(self):
        """The installed IqLevel, or None while none is on."""
        return self._get_record(self._lib.gyp_ingest_get_level, IqLevel)

    def calibrate(self, first_ms: int = 0, n_ms: int = 100, target_rms: Optional[float] = None, remove_dc: bool = True,
                  clip_level: float = 0.0):
        """Measure output milliseconds [first_ms, first_ms + n_ms) of the handle's unconditioned output (word * scale, no level) on
        the device and install the level that removes their mean (remove_dc) and brings the RMS of |x| to target_rms (default:
        gypsum_amd.level.default_target_rms(N)).  Returns (IqLevel, measured) as gypsum_amd.level.level_from_stats does; the
        cursor stays where it was, blocks handed out earlier are no longer valid (gyp_ingest_calibrate)."""
        target = default_target_rms(self.n) if target_rms is None else float(target_rms)
        return self._find_record(self._lib.gyp_ingest_calibrate, IqLevel, first_ms, n_ms, int(bool(remove_dc)), target, float(clip_level))

    def set_notches(self, freqs_hz) -> None:
        """Tones (whole Hz, at most 8, |f| < fs / 2, 4000 Hz apart) projected out of every device block from the next block handed
        out on, between whatever produced the block and the level (gyp_ingest_set_notches).  None or an empty list switches them off."""
        f = np.zeros(0, dtype=np.int64) if freqs_hz is None else np.ascontiguousarray(freqs_hz, dtype=np.int64).reshape(-1)
        self._check(self._lib.gyp_ingest_set_notches(self._h, _lib.ptr(f) if len(f) else None, len(f)))

    @property
    def notches(self):
        """The installed tones in Hz, in the order they are removed (empty: none)."""
        f, n = np.zeros(_lib.GYP_NOTCH_MAX_TONES, dtype=np.int64), C.c_int32()
        self._check(self._lib.gyp_ingest_get_notches(self._h, _lib.ptr(f), C.byref(n)))
        return [int(x) for x in f[:n.value]]

    def find_tones(self, first_ms: int = 0, n_ms: int = 10, threshold: float = 16.0, max_tones: int = 8, install: bool = True):
        """Scan output milliseconds [first_ms, first_ms + n_ms) of the handle's output (no notches, no level) for CW tones on the
        device: a Hann spectrum over +-0.45 fs on a grid of fs / 2048, its local maxima `threshold` times above the median, each
        refined to a whole Hz.  Returns [(Hz, dB over the median), ...], strongest first, and installs them (install) as set_notches
        does; the cursor stays where it was, blocks handed out earlier are no longer valid (gyp_ingest_find_tones)."""
        f, db, n = np.zeros(_lib.GYP_NOTCH_MAX_TONES, dtype=np.int64), np.zeros(_lib.GYP_NOTCH_MAX_TONES), C.c_int32()
        self._check(self._lib.gyp_ingest_find_tones(self._h, int(first_ms), int(n_ms), float(threshold), int(max_tones), int(bool(install)),
                                                    _lib.ptr(f), _lib.ptr(db), C.byref(n)))
        return [(int(f[i]), float(db[i])) for i in range(n.value)]

    def set_blanker(self, blanker) -> None:
        """A gypsum_amd.blanker.Blanker every device block is blanked with from the next block handed out on, between whatever
        produced the block and the notches (gyp_ingest_set_blanker).  None switches it off."""
        self._set_record(self._lib.gyp_ingest_set_blanker, blanker)

    @property
    def blanker(self):
        """The installed Blanker, or None while none is on."""
        return self._get_record(self._lib.gyp_ingest_get_blanker, Blanker)

    def find_pulses(self, first_ms: int = 0, n_ms: int = 10, threshold_over_median: float = 16.0, guard: int = 4, remove_dc: bool = True,
                    install: bool = True):
        """Measure output milliseconds [first_ms, first_ms + n_ms) of the handle's output (no blanker, no notches, no level) on the
        device -- their mean as the centre (remove_dc; else 0), the histogram of the power about it -- and derive the blanker whose
        threshold is sqrt(threshold_over_median x the median power).  Returns (Blanker, measured) as
        gypsum_amd.blanker.blanker_from_hist does and installs it (install) as set_blanker does; the cursor stays where it was,
        blocks handed out earlier are no longer valid (gyp_ingest_find_pulses)."""
        return self._find_record(self._lib.gyp_ingest_find_pulses, Blanker, first_ms, n_ms, int(bool(remove_dc)), float(threshold_over_median),
                                 int(guard), int(bool(install)))

    def last_blanked(self) -> np.ndarray:
        """int32 counts of blanked samples per millisecond of the block most recently handed out by next_device_block (empty
        before the first block and after a seek; zeros while no blanker is on).  Waits for that block only (gyp_ingest_last_blanked)."""
        return self._last_counts(self._lib.gyp_ingest_last_blanked)

    def set_excisor(self, excisor) -> None:
        """A gypsum_amd.excisor.Excisor every device block is excised with from the next block handed out on, between the blanker
        and the notches (gyp_ingest_set_excisor).  None switches it off."""
        self._set_record(self._lib.gyp_ingest_set_excisor, excisor)

    def get_excisor(self):
        """The installed Excisor, or None while none is on (gyp_ingest_get_excisor)."""
        return self._get_record(self._lib.gyp_ingest_get_excisor, Excisor)

    excisor = property(get_excisor)

    def find_excisor(self, first_ms: int = 0, n_ms: int = 10, threshold_over_median: float = 16.0, guard: int = 1, install: bool = True):
        """Measure output milliseconds [first_ms, first_ms + n_ms) of the handle's output (behind the blanker where one is on; no
        excisor, no notches, no level) on the device -- the histogram of the bin powers of its 256-point frames -- and derive the
        excisor whose threshold is sqrt(threshold_over_median x the median power).  Returns (Excisor, measured) as
        gypsum_amd.excisor.excisor_from_hist does and installs it (install) as set_excisor does; the cursor stays where it was,
        blocks handed out earlier are no longer valid (gyp_ingest_find_excisor)."""
        return self._find_record(self._lib.gyp_ingest_find_excisor, Excisor, first_ms, n_ms, float(threshold_over_median), int(guard),
                                 int(bool(install)))

    def last_excised(self) -> np.ndarray:
        """int32 counts of excised (frame, bin) cells per millisecond of the block most recently handed out by next_device_block
        (empty before the first block and after a seek; zeros while no excisor is on).  Waits for that block only
        (gyp_ingest_last_excised)."""
        return self._last_counts(self._lib.gyp_ingest_last_excised)

    def seek(self, ms: int) -> None:
        self._check(self._lib.gyp_ingest_seek(self._h, int(ms)))

    def times(self, first_ms: int, n_ms: int) -> Tuple[np.ndarray, np.ndarray]:
        """chunk.start_time / chunk.end_time of each millisecond (antenna_sample_provider.py:88-96)."""
        start, end = np.empty(n_ms), np.empty(n_ms)
        self._check(self._lib.gyp_ingest_times(self._h, int(first_ms), int(n_ms), _lib.ptr(start), _lib.ptr(end)))
        return start, end

    def next_host_block(self) -> Optional[Tuple[int, np.ndarray]]:
        """(first_ms, words[n_ms, 2N] in the file's dtype) or None at the end.  The array is a view of the ring
        slot: it is overwritten by the next call."""
        raw, first, n_ms = C.c_void_p(), C.c_int64(), C.c_int32()
        self._check(self._lib.gyp_ingest_next_host(self._h, C.byref(raw), C.byref(first), C.byref(n_ms)))
        if n_ms.value == 0:
            return None
        count = n_ms.value * 2 * self.n
        buf = (C.c_char * (count * self.dtype.itemsize)).from_address(raw.value)
        return first.value, np.frombuffer(buf, dtype=self.dtype, count=count).reshape(n_ms.value, 2 * self.n)

    def next_device_block(self) -> Optional[Tuple[int, int, int]]:
        """(first_ms, n_ms, device pointer to complex64[n_ms * N]) or None at the end.  The engine's stream already
        waits for the upload; the block stays valid while the next depth-2 calls are made."""
        dev, first, n_ms = C.c_void_p(), C.c_int64(), C.c_int32()
        self._check(self._lib.gyp_ingest_next_dev(self._h, C.byref(dev), C.byref(first), C.byref(n_ms)))
        if n_ms.value == 0:
            return None
        return first.value, n_ms.value, dev.value
