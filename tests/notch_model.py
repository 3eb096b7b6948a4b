"""The notch in float64 numpy (include/gypsum_hip.h, "notch"): the measurement with exact phases, the sequential projection,
gyp_tones_find and gyp_tone_refine restated, and the scene of the end-to-end tests.  The yardstick of tests/test_notch_host.py and
tests/test_gpu_notch.py; nothing here runs on a device."""
from __future__ import annotations

import numpy as np

from gypsum_amd import synth

RECT, HANN = 0, 1
MIN_SEPARATION_HZ = 4000
MAX_TONES = 8


def phase_turns(f: int, first_index: int, count: int, fs: int) -> np.ndarray:
    """((f i) mod fs) / fs for i = first_index .. first_index + count - 1, reduced in exact integers (Python ints: any index)."""
    i0 = int(first_index) % int(fs)
    r = (int(f) % int(fs)) * ((i0 + np.arange(count, dtype=np.int64)) % int(fs)) % int(fs)      # both factors < 2^31
    return r.astype(np.float64) / float(fs)


def mixer(f: int, first_index: int, count: int, fs: int) -> np.ndarray:
    """e^(+j theta(i)) in complex128."""
    return np.exp(2j * np.pi * phase_turns(f, first_index, count, fs))


def window(kind: int, block: int) -> np.ndarray:
    if kind == RECT:
        return np.ones(block)
    return np.sin(np.pi * (np.arange(block) + 1.0) / (block + 1.0)) ** 2


def tones(x: np.ndarray, fs: int, freqs, block: int, kind: int = RECT, first_index: int = 0) -> np.ndarray:
    """A[b, k] = sum_n w[n] x[b B + n] e^(-j theta) / sum_n w[n] over the whole blocks of complex `x`, complex128."""
    x = np.asarray(x, dtype=np.complex128)
    n_blocks = len(x) // block
    w = window(kind, block)
    out = np.zeros((n_blocks, len(freqs)), dtype=np.complex128)
    for k, f in enumerate(freqs):
        m = np.conj(mixer(f, first_index, n_blocks * block, fs)).reshape(n_blocks, block)
        out[:, k] = (x[:n_blocks * block].reshape(n_blocks, block) * m * w).sum(axis=1) / w.sum()
    return out


def notch(x: np.ndarray, fs: int, n: int, freqs, first_index: int = 0):
    """The sequential projection per millisecond of n samples, in float64: (y complex128, A[n_ms, K] complex128)."""
    y = np.array(x, dtype=np.complex128)
    n_ms = len(y) // n
    amps = np.zeros((n_ms, len(freqs)), dtype=np.complex128)
    for t, f in enumerate(freqs):
        e = mixer(f, first_index, n_ms * n, fs).reshape(n_ms, n)
        rows = y[:n_ms * n].reshape(n_ms, n)
        a = (rows * np.conj(e)).mean(axis=1)
        amps[:, t] = a
        rows -= a[:, None] * e                     # (a view of y)
    return y, amps


def tones_find(power, threshold: float, min_separation_bins: int, max_tones: int):
    p = np.asarray(power, dtype=np.float64)
    bar = threshold * float(np.median(p))
    cand = [k for k in range(len(p))
            if p[k] >= bar and p[k] > 0 and (k == 0 or p[k] > p[k - 1]) and (k == len(p) - 1 or p[k] >= p[k + 1])]
    cand.sort(key=lambda k: (-p[k], k))
    out = []
    for k in cand:
        if len(out) >= max_tones:
            break
        if all(abs(k - j) >= min_separation_bins for j in out):
            out.append(k)
    return out


def refine(amps, block_seconds: float) -> float:
    a = np.asarray(amps, dtype=np.complex128)
    s = complex(0.0)
    for b in range(len(a) - 1):
        s += a[b + 1] * np.conj(a[b])
    return float(np.arctan2(s.imag, s.real) / (2.0 * np.pi * block_seconds))


def band_power(y: np.ndarray, fs: int, f_center: float, half_width_hz: float = 500.0) -> float:
    """Mean power per Hz-bin of `y` in f_center +- half_width_hz: the whole record's DFT evaluated on a 25 Hz grid, float64."""
    y = np.asarray(y, dtype=np.complex128)
    t = np.arange(len(y)) / float(fs)
    grid = f_center + np.arange(-half_width_hz, half_width_hz + 1e-9, 25.0)
    return float(np.mean([abs(np.sum(y * np.exp(-2j * np.pi * f * t)) / len(y)) ** 2 for f in grid]))


# ---------------------------------------------------------------------------------------------------- the scene
# 2.046 Msps, four planted satellites at the survey's a N = 20.46 and sigma = 5 a (synth.default_amplitudes), and a CW at
# +217 300 Hz whose amplitude is 40 dB above sigma (100 sigma).  Un-notched the oracle's acquisition misses planted satellites; on
# the model-notched samples it finds all four at their Doppler bins and code phases (tests/test_notch_host.py holds the gate).
SCENE_FS, SCENE_N = 2_046_000, 2046
SCENE_SATS = {5: (311, 1400.0), 12: (1530, -2100.0), 19: (902, 3500.0), 27: (64, -700.0)}      # sat: (code phase, Doppler Hz)
SCENE_TONE_HZ = 217_300
SCENE_TONE_DB = 40.0
SCENE_SEED = 217


def scene(n_ms: int = 10, tone_hz=(SCENE_TONE_HZ,), tone_db=(SCENE_TONE_DB,), seed: int = SCENE_SEED, tone_offset_hz: float = 0.0):
    """(x complex64 with the tones, its clean twin complex64): the same satellites and noise."""
    a, sigma = synth.default_amplitudes(SCENE_FS)
    sats = [synth.SyntheticSatellite(sat_id=sv, doppler_hz=d, code_phase=cp, carrier_phase=0.7 * sv, amplitude=a)
            for sv, (cp, d) in SCENE_SATS.items()]
    clean = synth.render(synth.SyntheticScene(fs=SCENE_FS, n_ms=n_ms, sats=sats, noise_sigma=sigma, seed=seed)).astype(np.complex128)
    i = np.arange(len(clean), dtype=np.float64)
    cw = np.zeros(len(clean), dtype=np.complex128)
    for k, (f, db) in enumerate(zip(tone_hz, tone_db)):
        cw += sigma * 10.0 ** (db / 20.0) * np.exp(1j * (2.0 * np.pi * ((f + tone_offset_hz) / SCENE_FS) * i + 0.4 + k))
    return (clean + cw).astype(np.complex64), clean.astype(np.complex64)


def scene_words(x: np.ndarray, q: float = None, peak: float = 120.0):
    """(int8 words, uint8 words + 128, LSB per unit): interleaved I,Q at q LSB per unit (default: the largest component at `peak`)."""
    if q is None:
        q = peak / float(max(np.abs(x.real).max(), np.abs(x.imag).max()))
    w = np.empty(2 * len(x))
    w[0::2], w[1::2] = x.real.astype(np.float64) * q, x.imag.astype(np.float64) * q
    w8 = np.clip(np.rint(w), -127, 127).astype(np.int8)
    return w8, (w8.astype(np.int16) + 128).astype(np.uint8), q
