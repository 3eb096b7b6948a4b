"""The resampler's host side (no GPU): the library's design against the float64 model of the contract, the model's own
passband accuracy, the refusals, and the rate helper."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from gypsum_amd import _lib
from gypsum_amd import resample as rs

import resample_model as model

PAIRS = [(2_048_000, 2_046_000), (4_000_000, 4_092_000), (5_000_000, 5_115_000), (10_000_000, 8_184_000),
         (20_000_000, 20_460_000), (25_000_000, 20_460_000), (16_368_000, 8_184_000), (50_000_000, 49_104_000)]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("fs_in,fs_out", PAIRS)
def test_design_matches_the_float64_model(fs_in, fs_out):
    got = rs.design(fs_in, fs_out)
    want = model.design(fs_in, fs_out)
    assert got.shape == want.shape == (model.n_phases(fs_in, fs_out), 32)
    assert np.abs(got.astype(np.float64) - want).max() <= 2e-7
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6


# The rate edges: exactly x2 (L = 2, M = 1), about x2 with gcd 1 (L = 2046), exactly 0.5 (L = 1), about 0.5 with gcd 1 (L = 8184).
EDGE_PAIRS = [(1_023_000, 2_046_000), (1_025_000, 2_046_000), (16_368_000, 8_184_000), (16_367_000, 8_184_000)]
TAPS = [16, 24, 32, 48, 64]


def _ulp32(v: np.ndarray) -> np.ndarray:
    """The float32 ulp of the binade that holds |v| (float64; normal float32 range)."""
    _, e = np.frexp(np.abs(v))
    return np.ldexp(1.0, e - 24)


@pytest.mark.parametrize("taps", TAPS)
@pytest.mark.parametrize("fs_in,fs_out", sorted(set(PAIRS + EDGE_PAIRS)))
def test_design_is_the_float64_model_rounded_to_float32(fs_in, fs_out, taps):
    """Every tap, the smallest edge taps included, is the float64 model's tap correctly rounded: |h32 - h64| <= ulp32(h64) / 2.
    The 1e-9 relative slack covers libm sin and the I0 power series against np.sinc and np.i0 in float64."""
    got = rs.design(fs_in, fs_out, taps)
    want = model.design(fs_in, fs_out, taps)
    assert got.shape == want.shape == (model.n_phases(fs_in, fs_out), taps)
    assert np.all(want != 0)
    err = np.abs(got.astype(np.float64) - want)
    bound = 0.5 * _ulp32(want) + 1e-9 * np.abs(want)
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    assert np.all(err <= bound), (worst, want[worst], got[worst])
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6


def test_phase_counts():
    for fs_in, fs_out, L in ((2_048_000, 2_046_000, 1023), (4_000_000, 4_092_000, 1023), (5_000_000, 5_115_000, 1023),
                             (10_000_000, 8_184_000, 1023), (50_000_000, 49_104_000, 3069)):
        assert rs.n_phases(fs_in, fs_out) == L


@pytest.mark.parametrize("taps", [16, 24, 48, 64])
def test_other_tap_counts_match_the_model(taps):
    got = rs.design(4_000_000, 4_092_000, taps)
    assert got.shape == (1023, taps)
    assert np.abs(got.astype(np.float64) - model.design(4_000_000, 4_092_000, taps)).max() <= 2e-7
    assert rs.design(4_000_000, 4_092_000, 0).tobytes() == rs.design(4_000_000, 4_092_000, 32).tobytes()


# Passband per tap count (the table in include/gypsum_hip.h), as a fraction of min(fs_in, fs_out), at a ratio near 1, near x2 up
# and exactly 0.5.  At 0.5 the T input taps span only T/2 output samples and the transition band is wider: T = 16 holds 0.12
# (8.8e-4 at 0.15), T = 32 holds 0.25 (7.6e-4 at 0.30, 3.2e-2 at 0.35).
BAND = {16: (0.25, 0.25, 0.12), 24: (0.3, 0.3, 0.2), 32: (0.35, 0.35, 0.25), 48: (0.35, 0.35, 0.3), 64: (0.35, 0.35, 0.35)}
BAND_PAIRS = [(4_000_000, 4_092_000), (1_025_000, 2_046_000), (16_368_000, 8_184_000)]


def _tone_error(fs_in, fs_out, taps, band):
    n_ms = 3
    n_in = fs_in // 1000
    t_in = np.arange((n_ms + 2) * n_in) / fs_in
    t_out = np.arange(n_ms * (fs_out // 1000)) / fs_out
    edge = 80   # outputs whose taps reach before sample 0 see the zero padding
    worst = 0.0
    for f in np.array([-1.0, -0.6, 0.0, 0.3, 1.0]) * band * min(fs_in, fs_out):
        x = np.exp(2j * np.pi * f * t_in + 0.3j)
        y = model.resample(x, fs_in, fs_out, 0, n_ms, taps)
        want = np.exp(2j * np.pi * f * t_out + 0.3j)
        worst = max(worst, np.abs(y - want)[edge:].max())
    return worst


@pytest.mark.parametrize("fs_in,fs_out,taps", list(dict.fromkeys([(a, b, 32) for a, b in PAIRS] +
                                                                   [(a, b, t) for t in TAPS for a, b in BAND_PAIRS])))
def test_model_passes_tones_within_the_passband(fs_in, fs_out, taps):
    """A complex tone at |f| <= band * min(fs_in, fs_out) comes through at the right instant with error <= 2e-4 of its amplitude
    (band: 0.35 at T = 32 away from a ratio of 0.5; BAND per tap count at the three ratios it is written for)."""
    if (fs_in, fs_out) in BAND_PAIRS:
        band = BAND[taps][BAND_PAIRS.index((fs_in, fs_out))]
    else:
        band = 0.25 if 2 * fs_out == fs_in else 0.35
    assert _tone_error(fs_in, fs_out, taps, band) <= 2e-4


def test_refusals(lib):
    table = np.empty(1023 * 32, dtype=np.float32)
    n = C.c_int32()
    call = lambda a, b, t: lib.gyp_resample_design(a, b, t, _lib.ptr(table), C.byref(n))
    assert call(4_000_000, 4_092_000, 32) == _lib.GYP_OK
    for a, b in ((4_000_500, 4_092_000), (4_000_000, 4_092_500), (0, 4_092_000), (-4_000_000, 4_092_000),
                 (4_092_000, 4_092_000), (2_000_000, 4_092_000 + 1000), (10_000_000, 4_092_000), (1_000_000, 2_046_000)):
        assert call(a, b, 32) == _lib.GYP_E_BAD_RATE, (a, b)
    assert call(2_046_000, 4_092_000, 32) == _lib.GYP_OK        # exactly 2
    assert call(8_184_000, 4_092_000, 32) == _lib.GYP_OK        # exactly 0.5
    for t in (-1, 8, 31, 33, 128):
        assert call(4_000_000, 4_092_000, t) == _lib.GYP_E_BAD_ARG, t
    with pytest.raises(_lib.GypsumHipError) as e:
        rs.design(4_092_000, 4_092_000)
    assert e.value.code == _lib.GYP_E_BAD_RATE


def test_nearest_supported_rate():
    for fs_in, want in ((2_048_000, 2_046_000), (4_000_000, 4_092_000), (5_000_000, 5_115_000), (10_000_000, 10_230_000),
                        (25_000_000, 20_460_000), (20_000_000, 20_460_000), (50_000_000, 49_104_000), (8_184_000, 8_184_000)):
        assert rs.nearest_supported_rate(fs_in) == want, fs_in
    assert rs.nearest_supported_rate(3_580_500) == 3_069_000    # ties go to the lower rate (3.069 and 4.092 both 511.5 kHz away)
    with pytest.raises(ValueError):
        rs.nearest_supported_rate(200_000_000)


def test_raw_input_file_info(tmp_path):
    from gypsum_amd.radio_input import InputFileInfo, InputFileType
    info = InputFileInfo.raw(tmp_path / "cap.bin", 4_000_000, np.int16)
    assert info.format is InputFileType.Raw and info.sdr_sample_rate == 4_000_000
    assert np.dtype(info.sample_component_data_type) == np.int16
    with pytest.raises(ValueError):
        InputFileInfo.raw(tmp_path / "cap.bin", 4_000_000, np.int32)
