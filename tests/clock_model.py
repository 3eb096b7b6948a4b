"""Receiver clocks for the tracking tests, and what the reference's own arithmetic costs late in a recording (numpy and stdlib only).

Every tracking kernel wipes the carrier off at absolute receiver time, exp(-i (2 pi f (t0 + n / fs) + phi)), with t0 the caller's
start time (tracker.py:271-281).  The reference forms 2 pi f t + phi per sample in float64: at t0 = one GPS week the argument is
~2e10 rad and its rounding ~2e-6 rad, independent from sample to sample.  That is the reference's OWN noise; a device that reduces
f t0 exactly cannot (and need not) reproduce it term for term.  This module provides
  * clocks()          the start / end arrays of the clock shapes the tests feed (offset, off the microsecond grid, gapped, per stream);
  * exact_start()     a small start time whose carrier has the exactly reduced phase of (f, t0): the oracle's exact-phase twin;
  * reference_noise() oracle against exact twin for one teacher-forced millisecond;
  * bound()           the bars of tests/test_gpu_clocks.py, from number formats and that noise alone;
  * twin_horizon()    the first millisecond at which the oracle's own float32-perturbed twin produces a different integer
                      (tests/test_clock_horizon.py: closed-loop parity with the reference is only defined near t = 0).
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from oracle import gypsum_oracle as orc

GPS_WEEK_S = 604_800.0
OFFGRID_S = 1.0 / 3.0 * 1e-6          # a third of a microsecond: f t0 is then not representable, so carrier_cycles()'s exact fma matters
FLOAT32_FLOOR = 1e-6                  # a little over twice the float32 floor of the prompt magnitudes on record (4.3e-7)
FLOAT64_FLOOR = 5e-14                 # the bar of early64 / late64 at t = 0 (tests/test_gpu_dll_exact.py)


def clocks(n: int, fs: int, n_ms: int, kind: str, T=0.0, first_ms: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(start, end) of n_ms consecutive chunks, the first one millisecond `first_ms` of the recording.
    kind "offset"      orc.chunk_times + T (T a number of seconds);
         "offgrid"     the same + OFFGRID_S;
         "gapped"      the gapless clock with jumps: T = [(j, seconds), ...], every chunk from index j of the returned arrays on is
                       moved by `seconds` (jumps add up);
         "per_stream"  one offset per stream: T = [seconds, ...], arrays of shape (len(T), n_ms)."""
    base = np.array([orc.chunk_times((first_ms + j) * n, n, fs) for j in range(n_ms)], dtype=np.float64).reshape(n_ms, 2)
    start, end = base[:, 0].copy(), base[:, 1].copy()
    if kind == "offset":
        return start + float(T), end + float(T)
    if kind == "offgrid":
        return start + float(T) + OFFGRID_S, end + float(T) + OFFGRID_S
    if kind == "gapped":
        for j, dt in T:
            start[j:] += dt
            end[j:] += dt
        return start, end
    if kind == "per_stream":
        off = np.asarray(T, dtype=np.float64)[:, None]
        return start[None, :] + off, end[None, :] + off
    raise ValueError(kind)


def exact_start(f: float, t0: float) -> float:
    """A start time of a few hundred microseconds at most whose carrier is that of (f, t0) with frac(f t0) formed exactly:
    f * exact_start == frac(f t0) up to two roundings of a number below 1 (1e-16 cycles).  For ONE teacher-forced millisecond only: the
    loops' phase gain depends on the absolute time ("Clocks")."""
    if f == 0.0:
        return 0.0
    cycles = Fraction(f) * Fraction(t0)
    return float(cycles - math.floor(cycles)) / f


def ulp(x: float) -> float:
    return math.ulp(abs(x))


def oracle_ms(samples: np.ndarray, prn: np.ndarray, fs: int, n: int, f: float, phi: float, cp: int, t0: float) -> orc.TrackStepRecord:
    """One teacher-forced millisecond of the oracle from the state (f, phi, cp), with np.argmax's own margin recorded."""
    trk = orc.Tracker(orc.TrackingState(float(f), float(phi), int(cp)), prn, fs, n)
    trk.record_margins = True
    return trk.process_samples(samples, t0, t0 + orc.ONE_MILLISECOND)


def el_scale(samples: np.ndarray, n: int) -> float:
    """|single-lag sum| <= ||x|| * ||prn||: what tests/test_gpu_dll_exact.py normalises early / late with (|carrier| = 1)."""
    return float(np.sqrt(np.sum(np.abs(np.asarray(samples, dtype=np.complex128)) ** 2) * n))


def reference_noise(samples: np.ndarray, prn: np.ndarray, fs: int, n: int, f: float, phi: float, cp: int, t0: float,
                    rec: Optional[orc.TrackStepRecord] = None) -> Dict[str, float]:
    """The oracle's millisecond at t0 against its exact-phase twin (exact_start): "mag" relative |peak| difference, "angle" of the peak
    (rad), "peak" |complex difference| / |peak|, "strength" relative, "el" the worst of early / late over el_scale(), "disc" the absolute
    difference of the discriminators (a difference of two nearly equal squares: at one GPS week the reference's own value moves by
    3e-6 .. 7e-6 of itself); "twin" the twin's record itself.  A common rotation of early and late does not change the discriminator, so "disc" is per-sample noise only."""
    a = rec if rec is not None else oracle_ms(samples, prn, fs, n, f, phi, cp, t0)
    b = oracle_ms(samples, prn, fs, n, f, phi, cp, exact_start(f, t0))
    if a.peak_offset != b.peak_offset:         # (no excuse path: the callers assert an arg-max margin of 1e-5, which excludes this)
        raise ValueError(f"the oracle's arg-max at t0 = {t0} ({a.peak_offset}) is not its exact-phase twin's ({b.peak_offset})")
    scale = el_scale(samples, n)
    return {"mag": abs(abs(a.peak) - abs(b.peak)) / abs(b.peak),
            "angle": abs(float(np.angle(a.peak * np.conj(b.peak)))),
            "peak": abs(a.peak - b.peak) / abs(b.peak),
            "strength": abs(a.strength - b.strength) / b.strength,
            "el": max(abs(a.early - b.early), abs(a.late - b.late)) / scale,
            "disc": abs(a.discriminator - b.discriminator), "twin": b}


def bound(T: float, f: float, what: str, noise: float = 0.0) -> float:
    """The bar on a device output at start time T and Doppler f, `noise` being reference_noise()'s share for the same quantity.
    what "f32": 1e-6 (float32 floor) + 4 pi ulp(|f| T) (the cycle count f t0 + phi / 2 pi rounded twice, in the product and in the add, half
                an ulp each, in radians) + noise;
         "f64": 5e-14 (the bar at t = 0) + 3 x noise (the reference's per-sample roundings are independent, so their worst case over a
                dozen lags fluctuates around the one measured)."""
    if what == "f32":
        return FLOAT32_FLOOR + 4.0 * math.pi * ulp(abs(f) * abs(T)) + noise
    if what == "f64":
        return FLOAT64_FLOOR + 3.0 * noise
    raise ValueError(what)


INTEGERS = ("pseudosymbol", "code_phase_after", "peak_offset", "locked")


def oracle_rows(iq: np.ndarray, prn: np.ndarray, fs: int, n: int, init: Sequence[float], start: np.ndarray, end: np.ndarray, first_ms: int,
                peak_noise: float = 0.0, margins: bool = False):
    """The oracle's records of one channel init = (doppler, carrier phase, code phase) over the chunks first_ms .. of `iq` on the clock
    (start, end); stops at a LostSatelliteLock / a zero pseudosymbol (the list is then shorter)."""
    trk = orc.Tracker(orc.TrackingState(float(init[0]), float(init[1]), int(init[2])), prn, fs, n)
    trk.peak_noise = peak_noise
    trk.record_margins = margins
    rows = []
    for j in range(len(start)):
        ms = first_ms + j
        try:
            rows.append(trk.process_samples(iq[ms * n:(ms + 1) * n], float(start[j]), float(end[j])))
        except (orc.LostSatelliteLock, KeyError):
            break
    return rows, trk


def twin_horizon(iq, prn, fs, n, init, start, end, first_ms, peak_noise: float = 3e-7):
    """(first index at which the oracle and its twin with float32-sized peak perturbations (orc.Tracker.peak_noise) differ in an integer,
    or None; worst Doppler separation in Hz over the common rows; rows of the oracle with locked = 1)."""
    a, _ = oracle_rows(iq, prn, fs, n, init, start, end, first_ms)
    b, _ = oracle_rows(iq, prn, fs, n, init, start, end, first_ms, peak_noise=peak_noise)
    first = None
    for j, (x, y) in enumerate(zip(a, b)):
        if any(getattr(x, k) != getattr(y, k) for k in INTEGERS):
            first = j
            break
    if first is None and len(a) != len(b):
        first = min(len(a), len(b))
    m = min(len(a), len(b)) if first is None else first
    sep = max((abs(x.doppler_after - y.doppler_after) for x, y in zip(a[:m], b[:m])), default=0.0)
    return first, sep, sum(int(r.locked) for r in a)


# ------------------------------------------------------------------ the scenes of tests/test_clock_horizon.py, shared with the closed loops
# of tests/test_gpu_clocks.py so that their length comes from the oracle alone
HORIZON_SEEDS = {"lock": 11, "pull-in": 12}
HORIZON_FIRST_MS = 9
HORIZON_N_MS = 200
_horizon_cache: Dict[tuple, tuple] = {}


def horizon_scene(fs: int, n_ms: int, regime: str):
    """(iq, [(sat_id, doppler, carrier phase, code phase)] of the first two channels) of the horizon scene of `regime`, `n_ms` long."""
    from gypsum_amd import synth
    import survey_worker

    n = fs // 1000
    seed = HORIZON_SEEDS[regime]
    if regime == "lock":
        scene = synth.lock_regime_scene(fs, n_ms, seed)
    else:
        scene = synth.random_scene(fs, n_ms, 2, seed, max_code_phase=(2046 if n > 2046 else None))
    inits = survey_worker.scene_inits(scene, np.random.default_rng(seed ^ 0x5EED))[:2]
    return synth.render(scene), inits


def horizons(fs: int, T: float, n_ms: int = HORIZON_N_MS):
    """Per channel of the two horizon scenes (lock regime first): (first differing index or None, Doppler separation, locked rows) of
    twin_horizon over n_ms milliseconds from HORIZON_FIRST_MS on the clock "offset" T."""
    key = (fs, float(T), n_ms)
    if key not in _horizon_cache:
        n = fs // 1000
        chips = orc.generate_ca_codes()
        start, end = clocks(n, fs, n_ms, "offset", T, HORIZON_FIRST_MS)
        out = []
        for regime in ("lock", "pull-in"):
            iq, inits = horizon_scene(fs, HORIZON_FIRST_MS + n_ms, regime)
            for sv, dop, phi, cp in inits:
                out.append(twin_horizon(iq, orc.prn_as_complex(chips[sv - 1], n), fs, n, (dop, phi, cp), start, end, HORIZON_FIRST_MS))
        _horizon_cache[key] = tuple(out)
    return _horizon_cache[key]


def horizon(fs: int, T: float, n_ms: int = HORIZON_N_MS) -> int:
    """Milliseconds from HORIZON_FIRST_MS for which every channel of the horizon scenes agrees with its float32-perturbed twin on every
    integer (n_ms: no twin differs)."""
    return min(n_ms if h[0] is None else h[0] for h in horizons(fs, T, n_ms))
