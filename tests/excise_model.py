"""The excisor in numpy (include/gypsum_hip.h, "excisor"): framing, the periodic Hann window, the spectra, the hit / circular guard
/ subtract rule in float64, the bin-power histogram, gyp_excise_from_hist's arithmetic, a float32 restatement (numpy's transform of
complex64 runs in single precision) that the GPU tests take their tolerances from, and the two scenes of the end-to-end tests.
The yardstick of tests/test_excise_host.py and tests/test_gpu_excise.py; nothing here runs on a device."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import blank_model
import notch_model

FRAME, HOP = 256, 128
BINS = blank_model.BINS
MAX_GUARD = 8


class Excisor(NamedTuple):
    threshold: float      # a float32 value
    guard: int


def n_frames(n: int) -> int:
    return (n + HOP + HOP - 1) // HOP


def full_frames(n: int) -> np.ndarray:
    """The frames that lie entirely inside a millisecond of n samples: f >= 1 and 128 f + 128 <= n."""
    return np.arange(1, max(n // HOP - 1, 0) + 1)


def window() -> np.ndarray:
    """w[k] = sin^2(pi k / 256), float64 rounded to float32."""
    return (np.sin(np.pi * np.arange(FRAME) / FRAME) ** 2).astype(np.float32)


def frames(row: np.ndarray) -> np.ndarray:
    """[nf, 256]: frame f is samples 128 f - 128 .. 128 f + 127 of the millisecond `row`, zeros outside it."""
    n, nf = len(row), n_frames(len(row))
    padded = np.zeros((nf + 1) * HOP, dtype=row.dtype)
    padded[HOP:HOP + n] = row
    return np.stack([padded[f * HOP:f * HOP + FRAME] for f in range(nf)])


def spectra(row: np.ndarray) -> np.ndarray:
    """complex128 [nf, 256]: X_f = FFT256(w x_f) of one millisecond, not normalised."""
    return np.fft.fft(frames(np.asarray(row, dtype=np.complex64).astype(np.complex128)) * window().astype(np.float64), axis=1)


def dilate(hit: np.ndarray, guard: int) -> np.ndarray:
    """[.., 256] bool: every bin within `guard` of a hit, round the ring of 256."""
    cut = hit.copy()
    for s in range(1, guard + 1):
        cut |= np.roll(hit, s, axis=-1) | np.roll(hit, -s, axis=-1)
    return cut


def pack_masks(cut: np.ndarray) -> np.ndarray:
    """[.., 256] bool -> [.., 4] uint64: bit k & 63 of word k >> 6 is bin k."""
    bits = cut.reshape(cut.shape[:-1] + (4, 64)).astype(np.uint64)
    return (bits << np.arange(64, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


def unpack_masks(words: np.ndarray) -> np.ndarray:
    w = np.asarray(words, dtype=np.uint64)
    return (((w[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)) != 0).reshape(w.shape[:-1] + (FRAME,))


def _excise(x, n, excisor, masks, ctype, ftype):
    x = np.asarray(x, dtype=np.complex64)
    y = x.copy()
    n_ms, nf = len(x) // n, n_frames(n)
    w = window().astype(ftype)
    with np.errstate(over="ignore"):
        t2 = np.float32(excisor.threshold) * np.float32(excisor.threshold)
    out_masks = np.zeros((n_ms, nf, 4), dtype=np.uint64)
    counts = np.zeros(n_ms, dtype=np.int32)
    for m in range(n_ms):
        row = x[m * n:(m + 1) * n]
        with np.errstate(invalid="ignore", over="ignore"):
            X = np.fft.fft(frames(row.astype(ctype)) * w, axis=1)
            assert X.dtype == ctype
            if masks is None:
                re, im = X.real.astype(np.float32), X.imag.astype(np.float32)
                a, b = re * re, im * im
                cut = dilate((a + b) >= t2, int(excisor.guard))     # NaN compares false
            else:
                cut = unpack_masks(masks[m])
            out_masks[m] = pack_masks(cut)
            counts[m] = int(cut.sum())
            corr = np.zeros((nf + 1) * HOP, dtype=ctype)
            touched = np.zeros((nf + 1) * HOP, dtype=bool)
            for f in np.flatnonzero(cut.any(axis=1)):               # the lower frame first
                e = (np.fft.ifft(np.where(cut[f], X[f], 0), axis=0)).astype(ctype)
                corr[f * HOP:f * HOP + FRAME] += e
                touched[f * HOP:f * HOP + FRAME] = True
            keep = touched[HOP:HOP + n]
            sub = (row.astype(ctype) - corr[HOP:HOP + n]).astype(np.complex64)
        y[m * n:(m + 1) * n][keep] = sub[keep]
    return y, out_masks, counts


def excise(x: np.ndarray, n: int, excisor: Excisor, masks=None):
    """(y complex64, uint64 masks [n_ms, nf, 4], int32 counts [n_ms]) over the whole milliseconds of n samples, in float64; a
    trailing part is left as it is.  With `masks` given, those decisions are applied instead of the model's own.  A sample whose
    two frames excised nothing keeps its bits."""
    return _excise(x, n, excisor, masks, np.complex128, np.float64)


def excise32(x: np.ndarray, n: int, excisor: Excisor, masks=None):
    """The same in float32: complex64 arrays, numpy's single-precision transform."""
    return _excise(x, n, excisor, masks, np.complex64, np.float32)


def powers32(x: np.ndarray, n: int) -> np.ndarray:
    """float32 [n_ms, full frames, 256]: p_k of the frames inside their millisecond, from the float64 spectra rounded once."""
    x = np.asarray(x, dtype=np.complex64)
    out = []
    for m in range(len(x) // n):
        X = spectra(x[m * n:(m + 1) * n])[full_frames(n)]
        with np.errstate(invalid="ignore", over="ignore"):
            re, im = X.real.astype(np.float32), X.imag.astype(np.float32)
            a, b = re * re, im * im
            out.append(a + b)
    return np.stack(out)


def spectrum_hist(x: np.ndarray, n: int) -> np.ndarray:
    """uint32[2048]: the count of bin powers per bin = (bits of p without the sign) >> 20, full frames only."""
    bins = (powers32(x, n).view(np.uint32) & np.uint32(0x7FFFFFFF)) >> np.uint32(20)
    return np.bincount(bins.reshape(-1), minlength=BINS).astype(np.uint32)


def from_hist(h: np.ndarray, threshold_over_median: float = 16.0, guard: int = 1):
    """(Excisor, median, t): the blanker's float64 arithmetic."""
    b, median, t = blank_model.from_hist(h, 0j, threshold_over_median, 0)
    return Excisor(b.threshold, int(guard)), median, t


# ---------------------------------------------------------------------------------------------------- the scenes
SCENE_FS, SCENE_N, SCENE_SATS = notch_model.SCENE_FS, notch_model.SCENE_N, notch_model.SCENE_SATS
JAMMER_DB = 40.0
FM_CARRIER_HZ, FM_INDEX, FM_RATE_HZ = 217_300, 20.0, 3000.0     # +-60 kHz deviation at a 3 kHz modulating rate
SWEEP_FROM_HZ, SWEEP_SPAN_HZ = -400e3, 800e3                    # over the whole scene: 80 kHz per millisecond at ten milliseconds


def jammer(kind: str, count: int, sigma: float) -> np.ndarray:
    i = np.arange(count, dtype=np.float64)
    amp = sigma * 10.0 ** (JAMMER_DB / 20.0)
    if kind == "fm":
        return amp * np.exp(1j * (2.0 * np.pi * FM_CARRIER_HZ / SCENE_FS * i + FM_INDEX * np.sin(2.0 * np.pi * FM_RATE_HZ / SCENE_FS * i)))
    if kind == "sweep":
        f = SWEEP_FROM_HZ + SWEEP_SPAN_HZ * i / count
        return amp * np.exp(1j * 2.0 * np.pi * np.cumsum(f) / SCENE_FS)
    raise ValueError(kind)


def scene(kind: str, n_ms: int = 10):
    """(x complex64 with the jammer, its clean twin complex64): notch_model's satellites and noise without its tone."""
    from gypsum_amd import synth
    _, clean = notch_model.scene(n_ms, tone_hz=(), tone_db=())
    _, sigma = synth.default_amplitudes(SCENE_FS)
    x = clean.astype(np.complex128) + jammer(kind, len(clean), sigma)
    return x.astype(np.complex64), clean
