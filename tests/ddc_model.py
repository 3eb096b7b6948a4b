"""Float64 model of the down-converter contract (include/gypsum_hip.h, "down-converter"), written from the contract alone.

    z[i] = x[i] exp(-j theta_i),  theta_i = 2 pi ((if_hz * i) mod fs_in) / fs_in   (i the absolute input index, exact integers)
    y    = sum_{j=-T/2+1..T/2} h_mu[j] z[i0 + j]     (i0, mu, h_mu: the resampler's, fc = 0.9 fs_out / fs_in)
"""
from __future__ import annotations

import numpy as np

import resample_model

TAPS = (32, 48, 64, 96, 128)


def rates_ok(fs_in: int, fs_out: int, if_hz: int) -> bool:
    """The acceptance rule, in Python integers."""
    if fs_in <= 0 or fs_out <= 0 or fs_in % 1000 or fs_out % 1000 or fs_in >= 2 ** 31:
        return False
    a = abs(if_hz)
    return 8 * fs_out >= fs_in and 20 * a >= 9 * fs_out and 20 * a + 9 * fs_out <= 10 * fs_in


def resolve_taps(fs_in: int, fs_out: int, taps: int = 0) -> int:
    """T = 0 -> the smallest of TAPS with T * fs_out >= 16 * fs_in."""
    if taps:
        return taps
    return next(t for t in TAPS if t * fs_out >= 16 * fs_in)


def design(fs_in: int, fs_out: int, taps: int) -> np.ndarray:
    """(L, T) float64, row p = mu * L: the resampler's design at fs_out < fs_in."""
    return resample_model.design(fs_in, fs_out, taps)


def mixer(fs_in: int, if_hz: int, first: int, n: int) -> np.ndarray:
    """exp(-j theta_i) for i = first .. first+n-1, the phase reduced exactly (Python integers: no overflow at any i)."""
    f = int(if_hz) % fs_in
    i0 = int(first) % fs_in
    idx = (np.arange(n, dtype=np.int64) + i0) % fs_in          # < 2^31
    r = (idx * f) % fs_in                                       # < 2^62: exact in int64
    return np.exp(-2j * np.pi * (r.astype(np.float64) / fs_in))


def mix(x: np.ndarray, fs_in: int, if_hz: int, x_first: int = 0) -> np.ndarray:
    """z = x * mixer: x[0] is input sample x_first."""
    return np.asarray(x, dtype=np.float64) * mixer(fs_in, if_hz, x_first, len(x))


def ddc(x: np.ndarray, fs_in: int, fs_out: int, if_hz: int, first_ms: int, n_ms: int, taps: int = 0,
        table: np.ndarray | None = None, x_first: int = 0) -> np.ndarray:
    """complex128 output milliseconds first_ms .. first_ms+n_ms-1 of the real recording x (zero outside it; x[0] is input
    sample x_first).  `table` (L, T) replaces the float64 design (e.g. the library's float32 one)."""
    T = resolve_taps(fs_in, fs_out, taps)
    return resample_model.resample(mix(x, fs_in, if_hz, x_first), fs_in, fs_out, first_ms, n_ms, T, table, x_first)


def abs_sums(x: np.ndarray, fs_in: int, fs_out: int, first_ms: int, n_ms: int, taps: int = 0, table: np.ndarray | None = None,
             x_first: int = 0) -> np.ndarray:
    """sum_j |h_j| |x_j| per output sample: the scale of the device's rounding of one component."""
    T = resolve_taps(fs_in, fs_out, taps)
    re, _ = resample_model.abs_sums(np.abs(np.asarray(x, dtype=np.float64)).astype(np.complex128), fs_in, fs_out, first_ms, n_ms, T,
                                    table, x_first)
    return re
