"""Models for the level tests (tests/test_level_host.py, tests/test_gpu_level.py): the per-millisecond statistics as numpy computes
them, a Python float64 restatement of gyp_iq_level_from_stats in the header's order, and the offset-binary scene of the end-to-end
test.  Python floats are IEEE doubles and every operator below is one rounding, which is what the header asks of the C function."""
from __future__ import annotations

import math

import numpy as np

from gypsum_amd import _lib, synth

GYP_E_BAD_ARG = _lib.GYP_E_BAD_ARG


def stats_of_words(words: np.ndarray, samples_per_ms: int, clip_level: float = 0.0) -> np.ndarray:
    """gyp_iq_stats records of interleaved I,Q integer `words` (one stream), sums in int64: exact."""
    w = np.asarray(words).astype(np.int64).reshape(-1, 2 * samples_per_ms)
    out = np.zeros(len(w), dtype=_lib.IQ_STATS)
    out["sum_re"] = w[:, 0::2].sum(axis=1)
    out["sum_im"] = w[:, 1::2].sum(axis=1)
    out["sum_sq"] = (w * w).sum(axis=1)
    out["max_abs"] = np.abs(w).max(axis=1)
    out["n_clip"] = (np.abs(w) >= clip_level).sum(axis=1) if clip_level > 0 else 0
    return out


def level_from_stats(stats: np.ndarray, samples_per_ms: int, remove_dc: bool, target_rms: float):
    """((dc_re, dc_im, gain) as float32, measured[4] as float64) in the order of include/gypsum_hip.h."""
    s_re = s_im = s_sq = 0.0
    c = 0
    for r in stats:
        s_re = s_re + float(r["sum_re"])
        s_im = s_im + float(r["sum_im"])
        s_sq = s_sq + float(r["sum_sq"])
        c += int(r["n_clip"])
    m = float(len(stats)) * float(samples_per_ms)
    m_re, m_im, p = s_re / m, s_im / m, s_sq / m
    d_re, d_im = (m_re, m_im) if remove_dc else (0.0, 0.0)
    a = d_re * d_re
    b = d_im * d_im
    q = a + b
    v = p - q
    rms = math.sqrt(v)
    g = float(target_rms) / rms
    level = np.array([d_re, d_im, g]).astype(np.float32)
    return level, np.array([m_re, m_im, rms, float(c) / (2.0 * m)])


# The scene of the end-to-end test: 2.046 Msps, satellites 3 / 11 / 22 at code phases 400 / 1200 / 77 and Doppler +1500 / -2750 / +310 Hz,
# a N = 30, sigma = 6 a, quantised to an RMS |x| of 20 LSB.
SCENE_FS, SCENE_N = 2_046_000, 2046
SCENE_SATS = {3: (400, 1500.0), 11: (1200, -2750.0), 22: (77, 310.0)}


def offset_binary_scene(n_ms: int = 12, seed: int = 20):
    """(int8 words w8, uint8 words w8 + 128, quantisation scale q in LSB per unit) of the scene, interleaved I,Q."""
    a = 30.0 / SCENE_N
    sats = [synth.SyntheticSatellite(sat_id=sv, doppler_hz=d, code_phase=cp, carrier_phase=0.3 * sv, amplitude=a)
            for sv, (cp, d) in SCENE_SATS.items()]
    x = synth.render(synth.SyntheticScene(fs=SCENE_FS, n_ms=n_ms, sats=sats, noise_sigma=6.0 * a, seed=seed)).astype(np.complex128)
    q = 20.0 / math.sqrt(float(np.mean(np.abs(x) ** 2)))
    words = np.empty(2 * len(x))
    words[0::2], words[1::2] = x.real * q, x.imag * q
    w8 = np.clip(np.rint(words), -127, 127).astype(np.int8)
    return w8, (w8.astype(np.int16) + 128).astype(np.uint8), q
