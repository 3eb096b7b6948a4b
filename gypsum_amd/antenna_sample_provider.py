"""Sample-provider interface (host mirror of `gypsum/antenna_sample_provider.py:20-136`).

The ABC, `SampleProviderAttributes`, `AntennaSampleChunk` and `NoMoreSamplesError`
keep the reference's names and semantics; `AntennaSampleProviderBackedByFile`
reads the same GNU Radio interleaved-float32 format with the same timestamps
(`round(cursor / fs, 6)`).  `AntennaSampleProviderBackedByArray` serves an
in-memory complex64 array (synthetic IQ) with identical chunking, which is what the
parity tests and the benchmark use since no recording is available offline.
"""
from __future__ import annotations

import ctypes as C
from abc import ABC, abstractmethod
from dataclasses import dataclass
from pathlib import Path

import numpy as np

PRN_REPETITIONS_PER_SECOND = 1000


class NoMoreSamplesError(Exception):
    pass


@dataclass
class SampleProviderAttributes:
    samples_per_second: int
    samples_per_prn_transmission: int


@dataclass
class AntennaSampleChunk:
    start_time: float
    end_time: float
    samples: np.ndarray


class AntennaSampleProvider(ABC):
    @abstractmethod
    def get_samples(self, sample_count: int) -> AntennaSampleChunk: ...

    @abstractmethod
    def peek_samples(self, sample_count: int) -> AntennaSampleChunk: ...

    @abstractmethod
    def seconds_since_start(self) -> float: ...

    @abstractmethod
    def get_attributes(self) -> SampleProviderAttributes: ...


class _CursorProvider(AntennaSampleProvider):
    sample_rate: float
    cursor: int
    utc_start_time: float

    def _elapsed(self, cursor: int) -> float:
        return round(cursor / self.sample_rate, 6)

    def seconds_since_start(self) -> float:
        return self._elapsed(self.cursor)

    def get_samples(self, sample_count: int) -> AntennaSampleChunk:
        chunk = self.peek_samples(sample_count)
        self.cursor += sample_count
        return chunk

    def get_block(self, n_ms: int) -> AntennaSampleChunk:
        """Up to `n_ms` whole milliseconds in one chunk (fewer at the end of the data; NoMoreSamplesError when none):
        what n_ms successive get_samples(N) calls would return, concatenated.  Not part of the reference's ABC."""
        n = int(self.sample_rate // PRN_REPETITIONS_PER_SECOND)
        parts = []
        start = self.seconds_since_start()
        for _ in range(n_ms):
            try:
                parts.append(self.get_samples(n).samples)
            except NoMoreSamplesError:
                if not parts:
                    raise
                break
        return AntennaSampleChunk(start_time=start, end_time=self.seconds_since_start(), samples=np.concatenate(parts))

    def get_attributes(self) -> SampleProviderAttributes:
        return SampleProviderAttributes(
            samples_per_second=int(self.sample_rate),
            samples_per_prn_transmission=int(self.sample_rate // PRN_REPETITIONS_PER_SECOND),
        )


class AntennaSampleProviderBackedByFile(_CursorProvider):
    """GNU Radio recording: interleaved float32 I/Q (antenna_sample_provider.py:79-136).

    `block_ms > 0` serves the usual one-millisecond chunks out of blocks read by the native reader thread
    (`gypsum_amd.ingest.IqFileIngest`, host-only mode) instead of opening the file and `np.fromfile`-ing it for
    every millisecond (:112-117); chunks, timestamps and the end-of-data condition are unchanged."""

    def __init__(self, path, sample_rate: float | None = None, utc_start_time: float = 0.0,
                 sample_component_data_type=np.float32, block_ms: int = 0) -> None:
        if hasattr(path, "sdr_sample_rate"):          # the reference's signature: one InputFileInfo (:80-86)
            info = path
            path, sample_rate = info.path, info.sdr_sample_rate
            utc_start_time = info.utc_start_time.timestamp()
            sample_component_data_type = info.sample_component_data_type
        if sample_rate is None:
            raise TypeError("sample_rate is required when no InputFileInfo is given")
        self.path = Path(path)
        self.cursor = 0
        self.sample_rate = sample_rate
        self.utc_start_time = utc_start_time
        self.sample_component_data_type = sample_component_data_type
        self.file_size_in_bytes = self.path.stat().st_size
        self._reader = None
        self._block_first_ms = 0
        self._block: np.ndarray | None = None
        if block_ms > 0:
            from .ingest import IqFileIngest
            self._reader = IqFileIngest(self.path, int(sample_rate), sample_component_data_type, block_ms=block_ms)

    def _words_from_reader(self, sample_count: int) -> np.ndarray | None:
        n = self._reader.n
        if sample_count != n or self.cursor % n:
            return None                              # not a whole aligned millisecond: use the plain path
        ms = self.cursor // n
        if ms >= self._reader.total_ms:
            return None                              # the plain path raises NoMoreSamplesError
        if self._block is None or not (self._block_first_ms <= ms < self._block_first_ms + len(self._block)):
            if self._block is None or ms != self._block_first_ms + len(self._block):
                self._reader.seek(ms)
            got = self._reader.next_host_block()
            if got is None:
                return None
            self._block_first_ms, self._block = got[0], got[1].copy()
        return self._block[ms - self._block_first_ms]

    def peek_samples(self, sample_count: int) -> AntennaSampleChunk:
        word_bytes = np.dtype(self.sample_component_data_type).itemsize
        start = self.cursor * 2 * word_bytes
        end = start + sample_count * 2 * word_bytes
        if end >= self.file_size_in_bytes:   # same (off-by-one-conservative) bound as the reference, :106
            raise NoMoreSamplesError(f"Ran out of samples at {self.seconds_since_start():.2f}s")
        words = self._words_from_reader(sample_count) if self._reader is not None else None
        if words is None:
            words = np.fromfile(self.path.as_posix(), dtype=self.sample_component_data_type,
                                count=sample_count * 2, offset=start)
        return AntennaSampleChunk(
            start_time=self.seconds_since_start(),
            end_time=self._elapsed(self.cursor + sample_count),
            samples=(words[0::2]) + (1j * words[1::2]),
        )


class AntennaSampleProviderBackedByArray(_CursorProvider):
    """In-memory complex64 IQ with the file provider's chunk/timestamp semantics."""

    def __init__(self, iq: np.ndarray, sample_rate: float, utc_start_time: float = 0.0) -> None:
        self.iq = np.ascontiguousarray(iq, dtype=np.complex64)
        self.cursor = 0
        self.sample_rate = sample_rate
        self.utc_start_time = utc_start_time

    def get_block(self, n_ms: int) -> AntennaSampleChunk:
        n = int(self.sample_rate // PRN_REPETITIONS_PER_SECOND)
        k = min(n_ms, (len(self.iq) - self.cursor) // n)
        if k <= 0:
            raise NoMoreSamplesError(f"Ran out of samples at {self.seconds_since_start():.2f}s")
        chunk = self.peek_samples(k * n)
        self.cursor += k * n
        return chunk

    def peek_samples(self, sample_count: int) -> AntennaSampleChunk:
        if self.cursor + sample_count > len(self.iq):
            raise NoMoreSamplesError(f"Ran out of samples at {self.seconds_since_start():.2f}s")
        return AntennaSampleChunk(
            start_time=self.seconds_since_start(),
            end_time=self._elapsed(self.cursor + sample_count),
            samples=self.iq[self.cursor:self.cursor + sample_count],
        )


class AntennaSampleProviderResampled(_CursorProvider):
    """A recording at any whole-kHz rate served at a supported rate (gypsum_amd.resample): the file is read by the native
    reader and resampled on the device (`gyp_ingest_open_resampled`); whole aligned output milliseconds come back through
    `get_samples(N)` / `get_block(n_ms)` with the usual timestamps (round(cursor / fs_out, 6)) and NoMoreSamplesError after
    the input file's `total_ms` milliseconds.  `get_attributes()` reports the output rate, so `GpsReceiver` and
    `BatchedGpsReceiver` run on it unchanged.

    `path` may be an `InputFileInfo` (e.g. `InputFileInfo.raw(path, 4_000_000, np.int16)`); `resample_to` defaults to
    `nearest_supported_rate(sample_rate)`; `scale` multiplies integer words (an 8-bit front end wants about 1/100, see
    gyp_ingest_set_scale).

    A real recording at an intermediate frequency (`InputFileInfo.real_if(...)`, or `if_hz=`) is down-converted to complex
    baseband instead (`gyp_ingest_open_ddc`); `resample_to` then defaults to `default_ddc_rate(sample_rate, if_hz)` and `taps`
    to the down-converter's automatic choice.

    A recording of 1-, 2- or 4-bit packed words (`InputFileInfo.packed(...)`, or `packing=`, gypsum_amd.packing) is unpacked on
    the device (`gyp_ingest_open_packed`).  With a packing, and only then, `resample_to` may equal the input rate (an I,Q
    recording at a supported rate, the default `resample_to` then): its words are only unpacked.

    `level` (a gypsum_amd.level.IqLevel) or `calibrate` (a dict of `IqFileIngest.calibrate`'s arguments, `{}` for its defaults;
    applied once after opening) removes a DC offset and normalises the amplitude of every sample served: what an offset-binary
    uint8 recording needs before it can be acquired.  The two exclude each other.

    `notches` (a list of whole Hz) or `find_tones` (True, or a dict of `IqFileIngest.find_tones`'s arguments; applied once after
    opening) removes CW interference from every sample served (gypsum_amd.notch); the two exclude each other.  The chain is
    producer -> notches -> level, and tones are found and installed BEFORE `calibrate` measures: its level is the notched output's.

    `blank` (a gypsum_amd.blanker.Blanker) or `find_pulses` (True, or a dict of `IqFileIngest.find_pulses`'s arguments; applied once
    after opening) blanks pulsed interference in every sample served (gypsum_amd.blanker); the two exclude each other.  The blanker
    stands in front of the notches and runs FIRST: tones and level are then measured on the blanked output.  Where `find_pulses`
    names no guard it is half the filter's taps (at most 64): a T-tap resampler or down-converter smears a pulse over T samples.

    `excise` (a gypsum_amd.excisor.Excisor) or `find_excisor` (True, or a dict of `IqFileIngest.find_excisor`'s arguments; applied
    once after opening, behind `find_pulses`) excises narrowband and swept interference that is no pure tone from every sample served
    (gypsum_amd.excisor); the two exclude each other.  The excisor stands behind the blanker and in front of the notches: tones and
    level are then measured on the excised output."""

    def __init__(self, path, sample_rate: float | None = None, resample_to: int | None = None, utc_start_time: float = 0.0,
                 sample_component_data_type=np.float32, scale: float = 1.0, taps: int | None = None, block_ms: int = 250,
                 engine=None, device: int = 0, if_hz: int | None = None, packing=None, level=None, calibrate: dict | None = None,
                 notches=None, find_tones=None, blank=None, find_pulses=None, excise=None, find_excisor=None) -> None:
        from .engine import GypsumEngine
        from .ingest import IqFileIngest
        from .resample import DEFAULT_TAPS, ddc_design, default_ddc_rate, nearest_supported_rate

        if hasattr(path, "sdr_sample_rate"):
            info = path
            path, sample_rate = info.path, info.sdr_sample_rate
            utc_start_time = info.utc_start_time.timestamp()
            sample_component_data_type = info.sample_component_data_type
            if if_hz is None:
                if_hz = getattr(info, "if_hz", None)
            if packing is None:
                packing = getattr(info, "packing", None)
        if sample_rate is None:
            raise TypeError("sample_rate is required when no InputFileInfo is given")
        if level is not None and calibrate is not None:
            raise ValueError("level and calibrate exclude each other: a level is either given or measured")
        if notches is not None and find_tones:
            raise ValueError("notches and find_tones exclude each other: tones are either given or found")
        if blank is not None and find_pulses:
            raise ValueError("blank and find_pulses exclude each other: a blanker is either given or measured")
        if excise is not None and find_excisor:
            raise ValueError("excise and find_excisor exclude each other: an excisor is either given or measured")
        self.path = Path(path)
        self.input_sample_rate = int(sample_rate)
        self.if_hz = None if if_hz is None else int(if_hz)
        self.packing = packing
        if resample_to is not None:
            self.sample_rate = int(resample_to)
        elif self.if_hz is not None:
            self.sample_rate = default_ddc_rate(self.input_sample_rate, self.if_hz)
        else:
            self.sample_rate = nearest_supported_rate(self.input_sample_rate)
        self.n = self.sample_rate // PRN_REPETITIONS_PER_SECOND
        self.cursor = 0
        self.utc_start_time = utc_start_time
        self.sample_component_data_type = sample_component_data_type
        if engine is None:
            engine = GypsumEngine(device)
            engine.set_stream_format(self.sample_rate, self.n)
            self._own_engine = True
        else:
            self._own_engine = False
        self.engine = engine
        if packing is not None:
            self._ingest = IqFileIngest(self.path, self.sample_rate, block_ms=block_ms, engine=engine, resample_from_hz=self.input_sample_rate,
                                        taps=taps, if_hz=self.if_hz, packing=packing)
            if scale != 1.0:
                self._ingest.set_scale(scale)
        else:
            self._ingest = IqFileIngest(self.path, self.sample_rate, sample_component_data_type, block_ms=block_ms, engine=engine,
                                        resample_from_hz=self.input_sample_rate, taps=taps, if_hz=self.if_hz)
            if np.dtype(sample_component_data_type) != np.dtype(np.float32) and scale != 1.0:
                self._ingest.set_scale(scale)
        self.blanker, self.pulses = blank, None  # pulses: {"median", "threshold"} where find_pulses ran
        if blank is not None:
            self._ingest.set_blanker(blank)
        elif find_pulses:
            args = dict(find_pulses) if isinstance(find_pulses, dict) else {}
            if "guard" not in args:
                if self.if_hz is not None:
                    filter_taps = ddc_design(self.input_sample_rate, self.sample_rate, self.if_hz, int(taps or 0)).shape[1]
                elif packing is not None and not packing.real and self.input_sample_rate == self.sample_rate:
                    filter_taps = 8                  # only unpacked: the blanker's own default guard of 4
                else:
                    filter_taps = int(taps or DEFAULT_TAPS)
                args["guard"] = min(filter_taps // 2, 64)
            self.blanker, self.pulses = self._ingest.find_pulses(**args)
        self.excisor, self.excised = excise, None  # excised: {"median", "threshold"} where find_excisor ran
        if excise is not None:
            self._ingest.set_excisor(excise)
        elif find_excisor:
            self.excisor, self.excised = self._ingest.find_excisor(**(find_excisor if isinstance(find_excisor, dict) else {}))
        self.tones = None                        # [(Hz, dB over the median), ...] where find_tones ran
        if notches is not None:
            self._ingest.set_notches(notches)
        elif find_tones:
            self.tones = self._ingest.find_tones(**(find_tones if isinstance(find_tones, dict) else {}))
        self.notches = self._ingest.notches
        self.level = level
        if level is not None:
            self._ingest.set_level(level)
        elif calibrate is not None:
            self.level, self.measured = self._ingest.calibrate(**calibrate)
        self.total_ms = self._ingest.total_ms
        self._block_first_ms = 0
        self._block: np.ndarray | None = None    # [n_ms, N] complex64, downloaded
        self._next_ms = 0                        # the first millisecond the ingest hands out next

    def _ms(self, ms: int) -> np.ndarray:
        if self._block is None or not (self._block_first_ms <= ms < self._block_first_ms + len(self._block)):
            if ms != self._next_ms:
                self._ingest.seek(ms)
            got = self._ingest.next_device_block()
            if got is None:
                raise NoMoreSamplesError(f"Ran out of samples at {self.seconds_since_start():.2f}s")
            first, count, dev = got
            host = np.empty((count, self.n), dtype=np.complex64)
            self.engine._check(self.engine.lib.gyp_memcpy_d2h(self.engine.ctx, host.ctypes.data_as(C.c_void_p), C.c_void_p(dev), host.nbytes))
            self._block_first_ms, self._block, self._next_ms = first, host, first + count
        return self._block[ms - self._block_first_ms]

    def peek_samples(self, sample_count: int) -> AntennaSampleChunk:
        if sample_count != self.n or self.cursor % self.n:
            raise ValueError(f"a resampled recording is served in whole aligned milliseconds ({self.n} samples)")
        ms = self.cursor // self.n
        if ms >= self.total_ms:
            raise NoMoreSamplesError(f"Ran out of samples at {self.seconds_since_start():.2f}s")
        return AntennaSampleChunk(start_time=self.seconds_since_start(), end_time=self._elapsed(self.cursor + sample_count),
                                  samples=self._ms(ms).copy())

    def get_block(self, n_ms: int) -> AntennaSampleChunk:
        if self.cursor % self.n:
            raise ValueError(f"a resampled recording is served in whole aligned milliseconds ({self.n} samples)")
        ms = self.cursor // self.n
        k = min(int(n_ms), self.total_ms - ms)
        if k <= 0:
            raise NoMoreSamplesError(f"Ran out of samples at {self.seconds_since_start():.2f}s")
        start = self.seconds_since_start()
        samples = np.concatenate([self._ms(ms + i) for i in range(k)])
        self.cursor += k * self.n
        return AntennaSampleChunk(start_time=start, end_time=self.seconds_since_start(), samples=samples)

    def close(self) -> None:
        if getattr(self, "_ingest", None) is not None:
            self._ingest.close()
            self._ingest = None
        if getattr(self, "_own_engine", False) and self.engine is not None:
            self.engine.close()
            self.engine = None
