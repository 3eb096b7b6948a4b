"""Recordings at any whole-kHz sample rate: the on-device resampler of libgypsum_hip (include/gypsum_hip.h, "resampler").

The engine runs at K x 1.023 Msps only.  A recording taken at a round rate (RTL-SDR 2.048 Msps, USRP / bladeRF 4, 5, 10, 20,
25 Msps) is turned on the device into a stream at a supported rate fs_out within a factor 2 of its own, by a fixed windowed-sinc
polyphase filter with zero delay; acquisition, tracking and bit decoding then run unchanged at fs_out.

    fs_out = nearest_supported_rate(4_000_000)          # 4_092_000
    engine.set_stream_format(fs_out, fs_out // 1000)
    ing = IqFileIngest(path, fs_out, np.int16, engine=engine, resample_from_hz=4_000_000)

Real-sampled recordings at an intermediate frequency (include/gypsum_hip.h, "down-converter") go through the same filter behind a
mixer: `ddc_output_rates(fs_in, if_hz)` lists the supported rates the rule admits and `default_ddc_rate` picks one.

    fs_out = default_ddc_rate(16_368_000, 4_092_000)    # 8_184_000
    ing = IqFileIngest(path, fs_out, np.int8, engine=engine, resample_from_hz=16_368_000, if_hz=4_092_000)
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


def _ddc_rates_ok(fs_in: int, fs_out: int, if_hz: int) -> bool:
    """The down-converter's rule (gyp_ddc_design), in integers."""
    if fs_in <= 0 or fs_out <= 0 or fs_in % 1000 or fs_out % 1000 or fs_in >= 2 ** 31:
        return False
    a = abs(int(if_hz))
    return 8 * fs_out >= fs_in and 20 * a >= 9 * fs_out and 20 * a + 9 * fs_out <= 10 * fs_in


def ddc_output_rates(fs_in: int, if_hz: int) -> tuple[int, ...]:
    """The supported rates (K x 1.023 Msps) a real recording at fs_in with its band at if_hz can be down-converted to, ascending."""
    return tuple(fs for fs in SUPPORTED_RATES if _ddc_rates_ok(int(fs_in), fs, int(if_hz)))


def default_ddc_rate(fs_in: int, if_hz: int) -> int:
    """The largest admitted rate <= 8.184 Msps, else the smallest admitted one; ValueError if the rule admits none."""
    rates = ddc_output_rates(fs_in, if_hz)
    if not rates:
        raise ValueError(f"no supported rate can be down-converted to from {fs_in} Hz at IF {if_hz} Hz")
    low = [fs for fs in rates if fs <= 8_184_000]
    return max(low) if low else min(rates)


def ddc_design(fs_in: int, fs_out: int, if_hz: int, taps: int = 0) -> np.ndarray:
    """The down-converter's float32 design, shape (L, T) in the resampler's layout; taps 0 resolves to the automatic T
    (host only, no GPU)."""
    lib = _lib.load()
    L, t = C.c_int32(), C.c_int32()
    rc = lib.gyp_ddc_design(int(fs_in), int(fs_out), int(if_hz), int(taps), None, C.byref(L), C.byref(t))
    if rc != 0:
        raise _lib.GypsumHipError(rc, (lib.gyp_last_error(None) or b"").decode())
    table = np.empty((L.value, t.value), dtype=np.float32)
    rc = lib.gyp_ddc_design(int(fs_in), int(fs_out), int(if_hz), int(taps), _lib.ptr(table), None, None)
    if rc != 0:
        raise _lib.GypsumHipError(rc, (lib.gyp_last_error(None) or b"").decode())
    return table
