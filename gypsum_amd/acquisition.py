"""`GpsSatelliteDetector` with the reference's interface (`gypsum/acquisition.py:44-219`), searched on the GPU.

Drop-in use inside the reference receiver (receiver.py:66):

    receiver.satellite_detector = gypsum_amd.acquisition.GpsSatelliteDetector(receiver.satellites_by_id)

`detect_satellites_in_antenna_data` runs the whole 10-level coarse-to-fine search of every requested satellite in
one `gyp_acquire` call (all satellites of a level share one kernel launch); the per-level method
`get_best_doppler_shift_estimation` is kept for callers that drive the levels themselves.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Any, Dict, List

import numpy as np

from ._lib import CELL_DESC, GYP_HYB_ALTERNATE, GYP_HYB_CODE_DOPPLER, GYP_NON_COHERENT, WEAK_MEASURED, WEAK_RESULT
from .antenna_sample_provider import SampleProviderAttributes
from .engine import default_engine
from .gps_ca_prn_codes import GpsSatelliteId
from .utils import IntegrationType, integrate_correlation_with_doppler_shifted_prn

_logger = logging.getLogger(__name__)

# config.py:7
ACQUISITION_INTEGRATED_CORRELATION_STRENGTH_DETECTION_THRESHOLD = 3

# The weak-signal search (detect_weak_satellites_in_antenna_data).  The default threshold on z is measured, not derived: the largest
# z of the float64 model on noise alone at the default configuration (2.046 Msps, 10-ms blocks, both flags, 200 ms, +-7 kHz, 32
# satellites) over 8 seeds was 10.75 (tools/hybrid_threshold.py; DESIGN.md lists the eight values), times 1.25.
DEFAULT_WEAK_Z_THRESHOLD = 13.4375
WEAK_SEARCH_SPREAD_HZ = 7000.0
WEAK_SEARCH_FINE_STEP_HZ = 10.0


@dataclass
class BestNonCoherentCorrelationProfile:
    doppler_shift: float
    non_coherent_correlation_profile: np.ndarray
    sample_offset_of_correlation_peak: int
    correlation_strength: float


@dataclass
class SatelliteAcquisitionAttemptResult:
    satellite_id: GpsSatelliteId
    doppler_shift: float
    carrier_wave_phase_shift: float
    prn_phase_shift: int
    correlation_strength: float


@dataclass
class WeakMeasurement:
    """What measure_weak_satellites reports per result (gyp_weak_measured beside the search's z): figures, not verdicts."""
    satellite_id: GpsSatelliteId
    doppler_shift: float             # Hz, refined
    carrier_wave_phase_shift: float  # radians at the buffer's first sample, modulo pi
    c0: int                          # code phase in 2^-40 chips at the centre of the buffer's first sample
    code_phase_samples: float        # the same as the sample, with its fraction, at which chip 0 begins: [0, N)
    bit_edge: int                    # a data-bit edge at every millisecond m with m % 20 == bit_edge
    cn0_dbhz: float                  # nan when the prompt's energy does not exceed the noise share
    dd_last: float                   # the last pass's correction in chips: the residual
    status: int                      # 0 ok; bit 1: no envelope above the noise in some pass
    correlation_strength: float      # the search's z
    record: np.ndarray               # the WEAK_MEASURED record itself (engine.weak_measured_state takes it)


def _sv(satellite_id: Any) -> int:
    return int(getattr(satellite_id, "id", satellite_id))


class GpsSatelliteDetector:
    def __init__(self, satellites_by_id: Dict[Any, Any], device: int = 0) -> None:
        self.satellites_by_id = satellites_by_id
        self._device = device

    def _engine(self, attrs: SampleProviderAttributes):
        return default_engine(attrs.samples_per_second, attrs.samples_per_prn_transmission, self._device)

    def _attempt_all(self, satellite_ids: List[Any], antenna_data: np.ndarray,
                     stream_attributes: SampleProviderAttributes) -> List[SatelliteAcquisitionAttemptResult]:
        n = stream_attributes.samples_per_prn_transmission
        n_ms = len(antenna_data) // n            # utils.py:36-37: only full blocks are integrated
        if n_ms == 0 or not satellite_ids:
            if satellite_ids:
                raise RuntimeError("Should never happen: Expected at least one correlation profile")
            return []
        rec = self._engine(stream_attributes).acquire(np.asarray(antenna_data)[:n_ms * n], 1, n_ms,
                                                      [_sv(s) for s in satellite_ids])
        return [SatelliteAcquisitionAttemptResult(
            satellite_id=sid, doppler_shift=int(r["doppler_hz"]), carrier_wave_phase_shift=float(r["carrier_phase"]),
            prn_phase_shift=int(r["code_phase"]), correlation_strength=float(r["strength"]))
            for sid, r in zip(satellite_ids, rec)]

    def detect_satellites_in_antenna_data(self, satellites_to_search_for: List[Any], antenna_data: np.ndarray,
                                          stream_attributes: SampleProviderAttributes) -> List[SatelliteAcquisitionAttemptResult]:
        """acquisition.py:52-68: results above the strength threshold, in search order."""
        detected = []
        for result in self._attempt_all(list(satellites_to_search_for), antenna_data, stream_attributes):
            if result.correlation_strength > ACQUISITION_INTEGRATED_CORRELATION_STRENGTH_DETECTION_THRESHOLD:
                _logger.info(f"Correlation strength above threshold, successfully detected satellite {result.satellite_id}!")
                detected.append(result)
        return detected

    def detect_weak_satellites_in_antenna_data(self, satellites_to_search_for: List[Any], antenna_data: np.ndarray,
                                               stream_attributes: SampleProviderAttributes, coherent_ms: int = 10, n_blocks: int | None = None,
                                               z_threshold: float = DEFAULT_WEAK_Z_THRESHOLD) -> List[SatelliteAcquisitionAttemptResult]:
        """Satellites too weak for detect_satellites_in_antenna_data (below about 38 dB-Hz): the hybrid coherent/non-coherent search of
        gyp_acquire_weak over n_blocks blocks of coherent_ms milliseconds (None: all the full blocks of antenna_data), alternating
        half-bit sets and code-Doppler alignment on, +-7 kHz coarse and 10 Hz fine.  Results with z above z_threshold, in search
        order; correlation_strength is z (NOT the strength the other method compares with 3)."""
        n = stream_attributes.samples_per_prn_transmission
        sats = list(satellites_to_search_for)
        if n_blocks is None:
            n_blocks = len(antenna_data) // (n * int(coherent_ms))
        if not sats or n_blocks < 2:
            if sats:
                raise RuntimeError("the weak-signal search needs at least two full blocks of coherent_ms milliseconds")
            return []
        iq = np.asarray(antenna_data)[:n_blocks * int(coherent_ms) * n]
        rec = self._engine(stream_attributes).acquire_weak(iq, 1, int(coherent_ms), int(n_blocks), GYP_HYB_ALTERNATE | GYP_HYB_CODE_DOPPLER,
                                                           [_sv(s) for s in sats], 0.0, WEAK_SEARCH_SPREAD_HZ, WEAK_SEARCH_FINE_STEP_HZ)
        return [SatelliteAcquisitionAttemptResult(
            satellite_id=sid, doppler_shift=float(r["doppler_hz"]), carrier_wave_phase_shift=float(r["carrier_phase"]),
            prn_phase_shift=int(r["code_phase"]), correlation_strength=float(r["z"]))
            for sid, r in zip(sats, rec) if float(r["z"]) > z_threshold]

    def refine_weak_satellites(self, results: List[SatelliteAcquisitionAttemptResult], antenna_data: np.ndarray,
                               stream_attributes: SampleProviderAttributes, first_ms: int = 0, params=None) -> List[SatelliteAcquisitionAttemptResult]:
        """Between detect_weak_satellites_in_antenna_data and a WeakSignalTracker: each result's Doppler refined to well below 1 Hz
        and its carrier phase re-estimated (gyp_weak_refine) from the whole milliseconds of antenna_data (40..2000: the search's own
        buffer or a longer one; its first sample is that of the search, millisecond first_ms of the recording).  One new result per
        input, in order, none dropped; a result whose peak lay at the edge of the scanned span (status 1) is logged."""
        results = list(results)
        if not results:
            return []
        n = stream_attributes.samples_per_prn_transmission
        n_ms = min(len(antenna_data) // n, 2000)
        cand = np.zeros(len(results), dtype=WEAK_RESULT)
        for c, r in zip(cand, results):
            c["sat_id"], c["doppler_hz"], c["carrier_phase"], c["code_phase"] = _sv(r.satellite_id), r.doppler_shift, r.carrier_wave_phase_shift, r.prn_phase_shift
        rec, _ = self._engine(stream_attributes).refine_weak(np.asarray(antenna_data)[:n_ms * n], 1, int(first_ms), cand, params)
        for r, o in zip(results, rec):
            log = _logger.warning if int(o["status"]) else _logger.info
            log(f"Weak hand-over of satellite {r.satellite_id}: Doppler {r.doppler_shift} -> {float(o['doppler_hz']):.2f} Hz, status {int(o['status'])}, "
                f"peak to mean {float(o['peak_to_mean']):.1f}, bit edge {int(o['edge'])}")
        return [SatelliteAcquisitionAttemptResult(
            satellite_id=r.satellite_id, doppler_shift=float(o["doppler_hz"]), carrier_wave_phase_shift=float(o["carrier_phase"]),
            prn_phase_shift=int(o["code_phase"]), correlation_strength=r.correlation_strength)
            for r, o in zip(results, rec)]

    def measure_weak_satellites(self, results: List[SatelliteAcquisitionAttemptResult], antenna_data: np.ndarray,
                                stream_attributes: SampleProviderAttributes, first_ms: int = 0, refine_params=None,
                                measure_params=None) -> List[WeakMeasurement]:
        """Between detect_weak_satellites_in_antenna_data and WeakSignalTracker.from_measurements: the hand-over (gyp_weak_refine: Doppler,
        carrier phase, bit edge) and then the measurement (gyp_weak_measure: the code phase to a fraction of a sample, the C/N0) of each
        result over the whole milliseconds of antenna_data (40..2000; its first sample is that of the search, millisecond first_ms of
        the recording).  One WeakMeasurement per input, in order, none dropped; a status other than 0 of either step is logged."""
        results = list(results)
        if not results:
            return []
        n = stream_attributes.samples_per_prn_transmission
        n_ms = min(len(antenna_data) // n, 2000)
        iq = np.asarray(antenna_data)[:n_ms * n]
        cand = np.zeros(len(results), dtype=WEAK_RESULT)
        for c, r in zip(cand, results):
            c["sat_id"], c["doppler_hz"], c["carrier_phase"], c["code_phase"] = _sv(r.satellite_id), r.doppler_shift, r.carrier_wave_phase_shift, r.prn_phase_shift
        eng = self._engine(stream_attributes)
        refined, _ = eng.refine_weak(iq, 1, int(first_ms), cand, refine_params)
        rec, _, _, _ = eng.measure_weak(iq, 1, int(first_ms), refined, measure_params)
        out = []
        for r, h, o in zip(results, refined, rec):
            log = _logger.warning if int(h["status"]) or int(o["status"]) else _logger.info
            log(f"Weak measurement of satellite {r.satellite_id}: Doppler {float(o['doppler_hz']):.2f} Hz, code phase {r.prn_phase_shift} -> "
                f"{float(o['code_phase_samples']):.3f} samples, residual {float(o['dd_last']):+.4f} chip, C/N0 {float(o['cn0_dbhz']):.1f} dB-Hz, "
                f"bit edge {int(o['edge'])}, status {int(h['status'])} / {int(o['status'])}")
            out.append(WeakMeasurement(
                satellite_id=r.satellite_id, doppler_shift=float(o["doppler_hz"]), carrier_wave_phase_shift=float(o["carrier_phase"]), c0=int(o["c0"]),
                code_phase_samples=float(o["code_phase_samples"]), bit_edge=int(o["edge"]), cn0_dbhz=float(o["cn0_dbhz"]), dd_last=float(o["dd_last"]),
                status=int(o["status"]), correlation_strength=r.correlation_strength, record=np.array(o, dtype=WEAK_MEASURED)))
        return out

    def _attempt_acquisition_for_satellite_id(self, satellite_id: Any, samples_for_integration_period: np.ndarray,
                                              stream_attributes: SampleProviderAttributes) -> SatelliteAcquisitionAttemptResult:
        return self._attempt_all([satellite_id], samples_for_integration_period, stream_attributes)[0]

    def get_best_doppler_shift_estimation(self, center_doppler_shift: float, doppler_shift_spread: float,
                                          antenna_data: np.ndarray, stream_attributes: SampleProviderAttributes,
                                          satellite_id: Any) -> BestNonCoherentCorrelationProfile:
        """acquisition.py:154-190: one level of the search, bins range(int(c-s), int(c+s), int(s/10)).

        The choice between bins goes through gyp_search_level: bins whose float32 maxima are within rounding of each
        other are re-evaluated in float64 on the device, as in the full search, so that the winner is the reference's."""
        n = stream_attributes.samples_per_prn_transmission
        n_ms = len(antenna_data) // n
        eng = self._engine(stream_attributes)
        iq = np.asarray(antenna_data)[:n_ms * n]
        level = eng.search_level(iq, 1, n_ms, [_sv(satellite_id)], center_doppler_shift, doppler_shift_spread)[0]
        cell = np.zeros(1, dtype=CELL_DESC)
        cell[0] = (0, _sv(satellite_id), float(level["doppler_hz"]), -1, 0)
        _, prof = eng.correlate_cells(iq, 1, n_ms, cell, GYP_NON_COHERENT, want_profiles=True)
        return BestNonCoherentCorrelationProfile(
            doppler_shift=int(level["doppler_hz"]), non_coherent_correlation_profile=prof[0].astype(np.float64),
            sample_offset_of_correlation_peak=int(level["code_phase"]), correlation_strength=float(level["strength"]))

    def get_integrated_correlation_with_doppler_shifted_prn(self, integration_type: IntegrationType, antenna_data: np.ndarray,
                                                            stream_attributes: SampleProviderAttributes, doppler_shift: float,
                                                            prn_as_complex: np.ndarray) -> np.ndarray:
        """acquisition.py:192-219 (the reference's cache is disabled there, `if False and ...`; none is kept here)."""
        return integrate_correlation_with_doppler_shifted_prn(integration_type, antenna_data, stream_attributes,
                                                              doppler_shift, prn_as_complex)
