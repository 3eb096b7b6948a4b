"""Tracking of the satellites the weak-signal search finds (GpsSatelliteDetector.detect_weak_satellites_in_antenna_data): a weak
bank (include/gypsum_hip.h, "weak-signal tracking") behind the reference's event type.

The reference's tracker emits one pseudosymbol per millisecond and leaves the bit edge and the bit value to its
NavigationBitIntegrator; at 30 dB-Hz a 1-ms pseudosymbol is a coin toss.  The weak bank integrates the 20 ms of a bit coherently
on the device, behind its own bit synchronisation, so a WeakSignalTracker hands out EmitNavigationBitEvents directly -- one per
channel per completed 20-ms period.  As in the reference until a preamble is matched, the polarity of a channel's bits is ambiguous
(a Costas loop locks at either half cycle): BitValue.ONE stands for a positive in-phase sum, nothing more.

The start must be close: from about 5 Hz of Doppler error the loop pulls in, from 7 or 8 Hz at 30 dB-Hz it usually settles in a
false lock, mostly 10 Hz or more off -- bits at chance, `mu` healthy (7.6 to 8.9 against 9 and above), status 0.  The weak search's 10-Hz fine
grid hands over either.  `phase_rms`, the rms of the PLL discriminator over the last 25 bits, tells the two apart: 0.13 to 0.30 rad in
lock and 0.74 to 1.06 rad in the false lock on the float64 model over nine scenes (tests/weak_track_scene.py prints them);
`WeakChannelStatus.false_lock` is phase_rms above FALSE_LOCK_PHASE_RMS = 0.5: that channel's bits are not to be used.  Nothing here
repairs it; the repair comes first: GpsSatelliteDetector.refine_weak_satellites brings the search's results within a fraction of a
hertz before they are handed to this class, and `bank.set_channel` restarts a slot from such a start.
"""
from __future__ import annotations

import collections
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._lib import CHAN_INIT
from ._records import WeakParams
from .acquisition import SatelliteAcquisitionAttemptResult
from .antenna_sample_provider import SampleProviderAttributes
from .engine import WeakChannelBank, default_engine, weak_measured_state
from .navigation_bit_intergrator import EmitNavigationBitEvent
from .tracker import BitValue


FALSE_LOCK_PHASE_RMS = 0.5      # radians; see the module's docstring
_PHASE_WINDOW = 25


def _sv(satellite_id) -> int:
    return int(getattr(satellite_id, "id", satellite_id))


def _ms_time(ms: int, n: int, fs: int) -> float:
    """The receiver timestamp at the start of millisecond `ms`, formed as the sample provider forms a chunk's:
    round(cursor / fs, 6) (antenna_sample_provider.py:92-96)."""
    return round(ms * n / fs, 6)


@dataclass
class WeakChannelStatus:
    satellite_id: object
    mu: float            # mean NBP / WBP of the last 25 periods; nan before 25 are complete
    doppler_hz: float    # the loop frequency
    status: int          # 0 tracking (or still synchronising), 2 lost or dropped
    phase: int           # 0 SYNC, 1 WAIT, 2 TRACK
    bit_edge: int        # 0..19 once found, else -1
    phase_rms: float = float("nan")   # rms of the PLL discriminator (radians) over the last 25 bits; nan before 25 are complete

    @property
    def false_lock(self) -> bool:
        """The loop is rotating through its discriminator, not holding the carrier: the bits are not to be used."""
        return self.phase_rms > FALSE_LOCK_PHASE_RMS


class WeakSignalTracker:
    """results: what detect_weak_satellites_in_antenna_data returned, taken at millisecond first_ms of the recording (the search's
    first sample).  process() takes the recording's next whole milliseconds and returns (channel index, EmitNavigationBitEvent) pairs
    in channel order, then time order; status() the per-channel mu, Doppler and status."""

    def __init__(self, results: Sequence[SatelliteAcquisitionAttemptResult], stream_attributes: SampleProviderAttributes,
                 params: Optional[WeakParams] = None, first_ms: int = 0, engine=None) -> None:
        if not results:
            raise ValueError("no acquisition results to track")
        self.attributes = stream_attributes
        self.n = int(stream_attributes.samples_per_prn_transmission)
        self.fs = int(stream_attributes.samples_per_second)
        self.satellite_ids = [r.satellite_id for r in results]
        inits = np.zeros(len(results), dtype=CHAN_INIT)
        for i, r in enumerate(results):
            inits[i] = (0, _sv(r.satellite_id), float(r.doppler_shift), float(r.carrier_wave_phase_shift), int(r.prn_phase_shift), 0)
        self._engine = engine if engine is not None else default_engine(self.fs, self.n)
        self.bank: WeakChannelBank = self._engine.create_weak_bank(inits, params, first_ms)
        self.cursor_ms = int(first_ms)
        self._dphi = [collections.deque(maxlen=_PHASE_WINDOW) for _ in results]

    @classmethod
    def from_measurements(cls, measurements: Sequence, stream_attributes: SampleProviderAttributes, first_ms: int = 0,
                          params: Optional[WeakParams] = None, ms_ahead: int = 0, engine=None) -> "WeakSignalTracker":
        """measurements: what GpsSatelliteDetector.measure_weak_satellites returned for a buffer whose first millisecond is
        first_ms of the recording.  Every channel is put in WAIT from its measured state (engine.weak_measured_state ->
        gyp_weak_bank_set_state): no SYNC, the first bit comes with the first whole data bit.  ms_ahead = 0: process() is given
        the recording from first_ms on (the measured buffer again, then what follows); ms_ahead = the buffer's milliseconds: from
        behind the buffer."""
        if not measurements:
            raise ValueError("no measurements to track")
        results = [SatelliteAcquisitionAttemptResult(satellite_id=m.satellite_id, doppler_shift=m.doppler_shift,
                                                     carrier_wave_phase_shift=m.carrier_wave_phase_shift,
                                                     prn_phase_shift=int(m.code_phase_samples), correlation_strength=m.correlation_strength)
                   for m in measurements]
        trk = cls(results, stream_attributes, params, int(first_ms) + int(ms_ahead), engine)
        for c, m in enumerate(measurements):
            st = weak_measured_state(m.record, trk.fs, trk.n, int(ms_ahead))
            trk.bank.set_state(c, float(st["f"]), float(st["f_int"]), float(st["u0"]), int(st["c0"]), int(st["edge"]))
        return trk

    def process(self, antenna_data: np.ndarray) -> List[Tuple[int, EmitNavigationBitEvent]]:
        x = np.asarray(antenna_data).reshape(-1)
        if x.size == 0 or x.size % self.n:
            raise ValueError("a whole, positive number of milliseconds of samples expected")
        events: List[Tuple[int, EmitNavigationBitEvent]] = []
        for at in range(0, x.size // self.n, 65535):                      # a call takes at most 65535 ms
            n_ms = min(65535, x.size // self.n - at)
            _, periods = self.bank.track_block(x[at * self.n:(at + n_ms) * self.n], 1, self.cursor_ms, n_ms, want_ms=False)
            self.cursor_ms += n_ms
            for c, recs in enumerate(periods):
                for r in recs:
                    self._dphi[c].append(float(r["dphi"]))
                    first = int(r["first_ms"])
                    events.append((c, EmitNavigationBitEvent(_ms_time(first, self.n, self.fs), _ms_time(first + 20, self.n, self.fs),
                                                             BitValue.ONE if int(r["bit"]) > 0 else BitValue.ZERO)))
        events.sort(key=lambda ce: ce[0])                                   # stable: time order within a channel stays
        return events

    def status(self) -> List[WeakChannelStatus]:
        st = self.bank.state()
        return [WeakChannelStatus(self.satellite_ids[c], float(s["mu_mean"]) if int(s["n_periods"]) >= 25 else float("nan"), float(s["f"]),
                                  int(s["status"]), int(s["phase"]), int(s["edge"]), self._phase_rms(c)) for c, s in enumerate(st)]

    def _phase_rms(self, channel: int) -> float:
        d = self._dphi[channel]
        return math.sqrt(sum(v * v for v in d) / len(d)) if len(d) == _PHASE_WINDOW else float("nan")
