"""A float64 model of the receiver loop (`gypsum/receiver.py:85-267`), built from the oracle's parts -- TEST INFRASTRUCTURE ONLY.

`ReceiverModel.step()` is one millisecond of `GpsReceiver.step()`: the chunk joins a rolling buffer of ten, the scan rule of
receiver.py:148-163 decides whether an acquisition runs over the eligible list (strength > `orc.ACQUISITION_STRENGTH_THRESHOLD`
keeps a satellite, acquisition.py:52-68), every acquired satellite gets a NEW `orc.Tracker` and a NEW `orc.BitIntegrator`, the tracked
satellites process the chunk in dict order, and one that raises `orc.LostSatelliteLock` is dropped and appended to the eligible list.
Timestamps are `orc.chunk_times`; "now" at the scan rule is the end of the current chunk (the provider's cursor has moved past it).

A tracker depends on nothing but its own acquisition result and the samples, so a life is run ahead to its loss (or to the end of
the scene) the moment it is acquired, and step() only consults what it recorded: the same receiver, millisecond for millisecond, but
the lives of one scan can run side by side in worker processes (`pool`, a multiprocessing pool of spawned workers; `None` runs
them in this process).

`ACQUISITION_SCAN_FREQUENCY` here and the oracle's `WATCHDOG_*` / `ACQUISITION_STRENGTH_THRESHOLD` are read when they are used, so a
test can patch them (tests/test_gpu_params.py::_patch); worker processes receive the values in force at that moment.
"""
from __future__ import annotations

import os

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")      # one BLAS thread per worker (tests/survey_worker.py says why)
os.environ.setdefault("OMP_NUM_THREADS", "1")

import contextlib
import math
import multiprocessing as mp
import sys
import tempfile
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

REPO = Path(__file__).resolve().parents[1]
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

from oracle import gypsum_oracle as orc  # noqa: E402

ACQUISITION_SCAN_FREQUENCY = 10          # config.py:9, seconds

_PATCHABLE = ("WATCHDOG_PERIOD_S", "WATCHDOG_DROP_BELOW", "WATCHDOG_NUDGE_BELOW", "WATCHDOG_NUDGE_HZ", "ACQUISITION_STRENGTH_THRESHOLD")


@dataclass
class Look:
    """One look of the circularity watchdog (tracker.py:370-387)."""
    step: int
    n_peaks: int
    circularity: Optional[float]     # None with fewer than two peaks (utils.py:134-137): the clock is stamped, nothing else happens
    action: str                      # "none", "nudge" or "drop"


@dataclass
class Life:
    """One satellite from an acquisition to its loss (or the end of the scene)."""
    sat_id: int
    acquired_at: int                             # the step whose scan acquired it; its first tracked millisecond
    acquisition: orc.AcquisitionResult
    records: List[orc.TrackStepRecord] = field(default_factory=list)      # one per millisecond that returned (not the one that raised)
    lost_at: Optional[int] = None
    bit_events: List[Tuple[float, float, int]] = field(default_factory=list)     # (first symbol start, last symbol end, orc.BIT_*)
    looks: List[Look] = field(default_factory=list)
    min_lock_margin: float = math.inf


@dataclass
class Scan:
    step: int
    sat_ids: List[int]                           # the eligible list handed to the detector, in order
    strengths: List[float]                       # per satellite of that list
    acquired: List[int]


def _constants() -> Dict[str, float]:
    return {k: getattr(orc, k) for k in _PATCHABLE}


def _chunk(iq, step: int, n: int) -> np.ndarray:
    return np.asarray(iq[step * n:(step + 1) * n])


def _open(iq):
    return np.load(iq, mmap_mode="r") if isinstance(iq, str) else iq


@contextlib.contextmanager
def shared_samples(iq: np.ndarray, n_jobs: int):
    """(path, pool): `iq` in a .npy file that worker processes map (under /dev/shm where there is one) and a pool of spawned
    workers, one per job and 16 at the most; the file is removed and the pool closed on the way out."""
    import survey_worker

    base = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    fd, path = tempfile.mkstemp(suffix=".npy", prefix="gyp_lifecycle_", dir=base)
    os.close(fd)
    try:
        np.save(path, iq)
        with mp.get_context("spawn").Pool(survey_worker.pool_size(n_jobs, cap=16)) as pool:
            yield path, pool
    finally:
        os.unlink(path)


def acquire_job(args) -> orc.AcquisitionResult:
    """acquisition.py:70-152 for one satellite on the ten chunks that end with `step`."""
    iq, fs, n, sat_id, step, consts = args
    for k, v in consts.items():
        setattr(orc, k, v)
    iq = _open(iq)
    data = np.asarray(iq[(step - orc.ACQUISITION_INTEGRATION_PERIOD_MS + 1) * n:(step + 1) * n])
    return orc.acquire_satellite(sat_id, data, fs, n, orc.prn_as_complex(orc.generate_ca_codes()[sat_id - 1], n))


def life_job(args) -> Life:
    """pipeline.py:56-79 + tracker.py:331-389 from the acquisition at `first` until the watchdog raises or the scene ends."""
    iq, fs, n, acq, first, n_steps, consts = args
    for k, v in consts.items():
        setattr(orc, k, v)
    iq = _open(iq)
    life = Life(acq.satellite_id, first, acq)
    trk = orc.Tracker(orc.TrackingState(acq.doppler_shift, acq.carrier_wave_phase_shift, acq.prn_phase_shift),
                      orc.prn_as_complex(orc.generate_ca_codes()[acq.satellite_id - 1], n), fs, n)
    trk.record_margins = True
    bits = orc.BitIntegrator()
    for step in range(first, n_steps):
        t0, t1 = orc.chunk_times(step * n, n, fs)
        looks = t0 - trk._last_circularity_check >= orc.WATCHDOG_PERIOD_S
        try:
            rec = trk.process_samples(_chunk(iq, step, n), t0, t1)
        except orc.LostSatelliteLock:
            rec = None
        if looks:          # the peaks the watchdog saw: this millisecond's included (tracker.py:346 runs before :370)
            peaks = np.array(trk.s.correlation_peaks_rolling_buffer)
            life.looks.append(Look(step, len(peaks), orc.constellation_circularity(peaks),
                                   "drop" if rec is None else "nudge" if rec.nudged else "none"))
        if rec is None:
            life.lost_at = step
            break
        life.records.append(rec)
        life.min_lock_margin = min(life.min_lock_margin, rec.lock_margin)
        life.bit_events.extend(bits.process(t0, rec.start_of_pseudosymbol, rec.end_of_pseudosymbol, rec.pseudosymbol)[1])
    return life


class ReceiverModel:
    def __init__(self, iq, fs: int, search_ids: List[int], n_steps: Optional[int] = None, pool=None) -> None:
        """`iq`: complex64 samples, or the path of a .npy file holding them (what worker processes open)."""
        self.iq_arg = iq
        self.iq = _open(iq)
        self.fs, self.n = fs, fs // 1000
        self.n_steps = len(self.iq) // self.n if n_steps is None else n_steps
        self.pool = pool
        self.eligible: List[int] = list(search_ids)
        self.tracked: Dict[int, Life] = {}                   # insertion order = tracking order (receiver.py:244)
        self.buffered = 0                                    # chunks in the rolling buffer, at most ten
        self.time_of_last_scan: Optional[float] = None
        self.steps_done = 0
        self.lives: Dict[int, List[Life]] = {}
        self.scans: List[Scan] = []
        self.changes: List[Tuple[int, List[int], List[int]]] = []     # (step, tracked ids, eligible list) after every change

    # receiver.py:148-163
    def _scan_if_due(self, step: int) -> None:
        now = orc.chunk_times(step * self.n, self.n, self.fs)[1]
        if self.time_of_last_scan is not None and now - self.time_of_last_scan < ACQUISITION_SCAN_FREQUENCY:
            return
        if self.buffered < orc.ACQUISITION_INTEGRATION_PERIOD_MS or not self.eligible:
            return                                           # the timestamp is NOT refreshed: it goes stale while the list is empty
        self.time_of_last_scan = now
        ids = list(self.eligible)
        consts = _constants()
        run = self.pool.map if self.pool is not None else lambda f, jobs: [f(j) for j in jobs]
        results = run(acquire_job, [(self.iq_arg, self.fs, self.n, sv, step, consts) for sv in ids])
        found = [r for r in results if r.correlation_strength > orc.ACQUISITION_STRENGTH_THRESHOLD]     # acquisition.py:52-68
        self.scans.append(Scan(step, ids, [float(r.correlation_strength) for r in results], [r.satellite_id for r in found]))
        for life in run(life_job, [(self.iq_arg, self.fs, self.n, r, step, self.n_steps, consts) for r in found]):
            self.tracked[life.sat_id] = life                 # a new pipeline: new tracker, new integrator (receiver.py:225-234)
            self.lives.setdefault(life.sat_id, []).append(life)
        self.eligible = [sv for sv in self.eligible if sv not in self.scans[-1].acquired]
        if found:
            self.changes.append((step, list(self.tracked), list(self.eligible)))

    def step(self) -> None:
        step = self.steps_done
        self.buffered = min(self.buffered + 1, orc.ACQUISITION_INTEGRATION_PERIOD_MS)
        self._scan_if_due(step)
        dropped = [sv for sv, life in self.tracked.items() if life.lost_at == step]      # receiver.py:237-257
        for sv in dropped:
            del self.tracked[sv]
            self.eligible.append(sv)
        if dropped:
            self.changes.append((step, list(self.tracked), list(self.eligible)))
        self.steps_done += 1

    def run(self) -> "ReceiverModel":
        while self.steps_done < self.n_steps:
            self.step()
        return self

    # ---------------------------------------------------------------- what the tests ask of a finished run
    def looks(self) -> List[Tuple[int, Look]]:
        return sorted(((sv, lk) for sv, ls in self.lives.items() for life in ls for lk in life.looks), key=lambda p: (p[1].step, p[0]))

    def margins(self) -> Dict[str, float]:
        """The smallest distances from a threshold this run saw (relative for the lock comparisons, absolute otherwise)."""
        circ = [lk.circularity for _, lk in self.looks() if lk.circularity is not None]
        thr = orc.ACQUISITION_STRENGTH_THRESHOLD
        return {
            "lock": min((life.min_lock_margin for ls in self.lives.values() for life in ls), default=math.inf),
            "circularity_drop": min((abs(c - orc.WATCHDOG_DROP_BELOW) for c in circ), default=math.inf),
            "circularity_nudge": min((abs(c - orc.WATCHDOG_NUDGE_BELOW) for c in circ), default=math.inf),
            "strength": min((abs(s - thr) for sc in self.scans for s in sc.strengths), default=math.inf),
        }

    def channel_ms(self) -> int:
        return sum(len(life.records) for ls in self.lives.values() for life in ls)
