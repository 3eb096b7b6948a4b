"""Float64 model of the resampler contract (include/gypsum_hip.h, "resampler"), written from the contract alone.

    i0 = m*N_in + floor(r*N_in / N_out),  mu = ((r*N_in) mod N_out) / N_out
    y  = sum_{j=-T/2+1..T/2} h_mu[j] x[i0 + j],  h_mu[j] = c(j - mu) / sum_j' c(j' - mu)
    c(t) = fc sinc(fc t) I0(beta sqrt(1 - (t/(T/2))^2)) / I0(beta),  fc = 0.9 min(fs_in, fs_out) / fs_in,  beta = 8
"""
from __future__ import annotations

from math import gcd

import numpy as np

RHO, BETA = 0.9, 8.0


def n_phases(fs_in: int, fs_out: int) -> int:
    n_in, n_out = fs_in // 1000, fs_out // 1000
    return n_out // gcd(n_in, n_out)


def taps_for(fs_in: int, fs_out: int, mu: np.ndarray, taps: int = 32) -> np.ndarray:
    """float64 h_mu[j], shape (len(mu), T), j = -T/2+1 .. T/2 along the last axis."""
    fc = RHO * min(fs_in, fs_out) / fs_in
    j = np.arange(-taps // 2 + 1, taps // 2 + 1, dtype=np.float64)
    t = j[None, :] - np.asarray(mu, dtype=np.float64)[:, None]
    c = fc * np.sinc(fc * t) * np.i0(BETA * np.sqrt(np.clip(1.0 - (t / (taps / 2)) ** 2, 0.0, None))) / np.i0(BETA)
    return c / c.sum(axis=1, keepdims=True)


def design(fs_in: int, fs_out: int, taps: int = 32) -> np.ndarray:
    """(L, T) float64, row p = mu * L."""
    L = n_phases(fs_in, fs_out)
    return taps_for(fs_in, fs_out, np.arange(L) / L, taps)


def _windows(x: np.ndarray, fs_in: int, fs_out: int, first_ms: int, n_ms: int, taps: int, table: np.ndarray | None,
             x_first: int):
    """Per output millisecond: (taps h[n, j] as float64, inputs x[n, j] as complex128), n over the ms's N_out samples."""
    n_in, n_out = fs_in // 1000, fs_out // 1000
    L = n_phases(fs_in, fs_out)
    h = design(fs_in, fs_out, taps) if table is None else np.asarray(table, dtype=np.float64)
    r = np.arange(n_out, dtype=np.int64)
    off = (r * n_in) // n_out
    row = ((r * n_in) % n_out) * L // n_out                 # mu * L, exact
    j = np.arange(-taps // 2 + 1, taps // 2 + 1, dtype=np.int64)
    x = np.asarray(x, dtype=np.complex128)
    for m in range(first_ms, first_ms + n_ms):
        idx = m * n_in + off[:, None] + j[None, :] - x_first
        ok = (idx >= 0) & (idx < len(x))
        yield h[row], np.where(ok, x[np.clip(idx, 0, max(len(x) - 1, 0))], 0)


def resample(x: np.ndarray, fs_in: int, fs_out: int, first_ms: int, n_ms: int, taps: int = 32, table: np.ndarray | None = None,
             x_first: int = 0) -> np.ndarray:
    """complex128 output milliseconds first_ms .. first_ms+n_ms-1 of the complex recording x (zero outside it).  `table`
    (L, T) replaces the float64 design (e.g. the library's float32 one, to isolate the arithmetic).  x[0] is input sample
    x_first: a short window stands in for a recording far from sample 0."""
    n_out = fs_out // 1000
    out = np.empty(n_ms * n_out, dtype=np.complex128)
    for k, (h, xs) in enumerate(_windows(x, fs_in, fs_out, first_ms, n_ms, taps, table, x_first)):
        out[k * n_out:(k + 1) * n_out] = (h * xs).sum(axis=1)
    return out


def abs_sums(x: np.ndarray, fs_in: int, fs_out: int, first_ms: int, n_ms: int, taps: int = 32, table: np.ndarray | None = None,
             x_first: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """(sum_j |h_j| |Re x_j|, sum_j |h_j| |Im x_j|) per output sample of resample(): the scale of a float32 chain's rounding."""
    n_out = fs_out // 1000
    re, im = np.empty(n_ms * n_out), np.empty(n_ms * n_out)
    for k, (h, xs) in enumerate(_windows(x, fs_in, fs_out, first_ms, n_ms, taps, table, x_first)):
        a = np.abs(h)
        re[k * n_out:(k + 1) * n_out] = (a * np.abs(xs.real)).sum(axis=1)
        im[k * n_out:(k + 1) * n_out] = (a * np.abs(xs.imag)).sum(axis=1)
    return re, im
