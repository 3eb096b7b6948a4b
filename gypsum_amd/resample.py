"""Recordings at any whole-kHz sample rate: the on-device resampler of libgypsum_hip (include/gypsum_hip.h, "resampler").

The engine runs at K x 1.023 Msps only.  A recording taken at a round rate (RTL-SDR 2.048 Msps, USRP / bladeRF 4, 5, 10, 20,
25 Msps) is turned on the device into a stream at a supported rate fs_out within a factor 2 of its own, by a fixed windowed-sinc
polyphase filter with zero delay; acquisition, tracking and bit decoding then run unchanged at fs_out.

    fs_out = nearest_supported_rate(4_000_000)          # 4_092_000
    engine.set_stream_format(fs_out, fs_out // 1000)
    ing = IqFileIngest(path, fs_out, np.int16, engine=engine, resample_from_hz=4_000_000)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

# the stream formats the engine runs at: K x 1.023 Msps (gyp_set_stream_format)
SUPPORTED_MULTIPLES = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 48)
SUPPORTED_RATES = tuple(1_023_000 * k for k in SUPPORTED_MULTIPLES)
DEFAULT_TAPS = 32


def nearest_supported_rate(fs_in: int) -> int:
    """The supported rate closest to `fs_in` among those within the resampler's ratio bounds (0.5 <= fs_out / fs_in <= 2),
    ties to the lower.  A supported `fs_in` is returned as it is (no resampling needed).  ValueError if none qualifies."""
    fs_in = int(fs_in)
    cands = [fs for fs in SUPPORTED_RATES if 2 * fs >= fs_in and fs <= 2 * fs_in]
    if fs_in <= 0 or not cands:
        raise ValueError(f"no supported rate within a factor 2 of {fs_in} Hz")
    return min(cands, key=lambda fs: (abs(fs - fs_in), fs))


def n_phases(fs_in: int, fs_out: int, taps: int = DEFAULT_TAPS) -> int:
    """L = N_out / gcd(N_in, N_out): the number of distinct filter phases."""
    lib = _lib.load()
    n = C.c_int32()
    rc = lib.gyp_resample_design(int(fs_in), int(fs_out), int(taps), None, C.byref(n))
    if rc != 0:
        raise _lib.GypsumHipError(rc, (lib.gyp_last_error(None) or b"").decode())
    return int(n.value)


def design(fs_in: int, fs_out: int, taps: int = DEFAULT_TAPS) -> np.ndarray:
    """The library's float32 design, shape (L, T): row p = mu * L holds h_mu[j] for j = -T/2+1 .. T/2 (host only, no GPU)."""
    lib = _lib.load()
    L = n_phases(fs_in, fs_out, taps)
    t = int(taps) or DEFAULT_TAPS
    table = np.empty((L, t), dtype=np.float32)
    rc = lib.gyp_resample_design(int(fs_in), int(fs_out), int(taps), _lib.ptr(table), None)
    if rc != 0:
        raise _lib.GypsumHipError(rc, (lib.gyp_last_error(None) or b"").decode())
    return table
