"""The pulse blanker in numpy (include/gypsum_hip.h, "blanker"): the float32 power and its eighth-octave histogram, gyp_blank_from_hist's
float64 arithmetic, the per-millisecond hit / guard / replace rule, and the pulsed scene of the end-to-end tests.  The yardstick of
tests/test_blank_host.py and tests/test_gpu_blank.py; nothing here runs on a device."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import notch_model

BINS = 2048
FINITE_BINS = 2040        # bins 0 .. 2039 hold the finite powers; +inf lands in 2040, NaN above
MAX_GUARD = 64


class Blanker(NamedTuple):
    center_re: float
    center_im: float
    threshold: float      # a float32 value
    guard: int


def power(x: np.ndarray, c=0j) -> np.ndarray:
    """p = (re - c_re)^2 + (im - c_im)^2 in float32, one rounding per operation."""
    x = np.asarray(x, dtype=np.complex64)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = x.real - np.float32(np.real(c))
        dy = x.imag - np.float32(np.imag(c))
        a = dx * dx
        b = dy * dy
        p = a + b
    assert p.dtype == np.float32
    return p


def hist(x: np.ndarray, c=0j) -> np.ndarray:
    """uint32[2048]: the count of samples per bin = (bits of p without the sign) >> 20."""
    bins = (power(x, c).view(np.uint32) & np.uint32(0x7FFFFFFF)) >> np.uint32(20)
    return np.bincount(bins, minlength=BINS).astype(np.uint32)


def bin_edges() -> np.ndarray:
    with np.errstate(invalid="ignore"):                     # (the edges above 2040 are NaN)
        return (np.arange(BINS + 1, dtype=np.uint32) << np.uint32(20)).view(np.float32).astype(np.float64)


def from_hist(h: np.ndarray, c=0j, threshold_over_median: float = 16.0, guard: int = 4):
    """(Blanker, median, t): float64 in the header's order."""
    h = np.asarray(h, dtype=np.uint32)
    edges = bin_edges()
    cum = np.cumsum(h[:FINITE_BINS].astype(np.float64))
    M = float(cum[-1])
    if not M > 0.0:
        raise ValueError("no sample of finite power")
    r = M / 2.0
    k = int(np.argmax(cum >= r))
    before = float(cum[k - 1]) if k else 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        part = (r - before) / float(h[k])
        step = np.float64(part) * (edges[k + 1] - edges[k])
        median = float(edges[k] + step)
        t = float(np.sqrt(np.float64(threshold_over_median) * np.float64(median)))
        t32 = np.float32(t)
    if not median > 0.0 or not np.isfinite(t32) or not t32 > 0:
        raise ValueError("the threshold does not fit float32")
    return Blanker(float(np.float32(np.real(c))), float(np.float32(np.imag(c))), float(t32), int(guard)), median, t


def blank(x: np.ndarray, n: int, blanker: Blanker):
    """(y complex64, int32 counts per millisecond) over the whole milliseconds of n samples; a trailing part is left as it is."""
    x = np.asarray(x, dtype=np.complex64)
    y = x.copy()
    n_ms = len(x) // n
    c = np.complex64(complex(blanker.center_re, blanker.center_im))
    with np.errstate(over="ignore"):
        t2 = np.float32(blanker.threshold) * np.float32(blanker.threshold)
    counts = np.zeros(n_ms, dtype=np.int32)
    g = int(blanker.guard)
    for m in range(n_ms):
        row = x[m * n:(m + 1) * n]
        with np.errstate(invalid="ignore"):
            hit = power(row, c) >= t2                       # NaN compares false
        # dilation by the guard inside the millisecond: a difference of the hits' running count
        run = np.concatenate([[0], np.cumsum(hit)])
        lo, hi = np.clip(np.arange(n) - g, 0, n), np.clip(np.arange(n) + g + 1, 0, n)
        gone = run[hi] > run[lo]
        y[m * n:(m + 1) * n][gone] = c
        counts[m] = int(gone.sum())
    return y, counts


def pulses(count: int, sigma: float, seed: int, period: int = 409, width: int = 41, db: float = 30.0, jitter: int = 120) -> np.ndarray:
    """complex128[count]: complex-Gaussian bursts of `width` samples, one per `period` samples at 0 .. jitter-1 samples into the
    period, `db` above a noise of `sigma` per component; zero elsewhere."""
    rng = np.random.default_rng(seed)
    out = np.zeros(count, dtype=np.complex128)
    amp = sigma * 10.0 ** (db / 20.0)
    for start in range(0, count, period):
        a = start + int(rng.integers(0, jitter))
        b = min(a + width, count)
        if a < count:
            out[a:b] = amp * (rng.standard_normal(b - a) + 1j * rng.standard_normal(b - a))
    return out


SCENE_FS, SCENE_N, SCENE_SATS = notch_model.SCENE_FS, notch_model.SCENE_N, notch_model.SCENE_SATS
PULSE_SEED = 31


def scene(n_ms: int = 10):
    """(x complex64 with the pulses, its clean twin complex64): notch_model's satellites and noise without its tone."""
    from gypsum_amd import synth
    _, clean = notch_model.scene(n_ms, tone_hz=(), tone_db=())
    _, sigma = synth.default_amplitudes(SCENE_FS)
    x = clean.astype(np.complex128) + pulses(len(clean), sigma, PULSE_SEED)
    return x.astype(np.complex64), clean
