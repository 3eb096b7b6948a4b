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


# At a ratio of exactly 0.5 the 32 input taps span only 16 output samples: the transition band reaches below 0.35 fs_out, and
# the tone test holds to 0.25 fs_out at T = 32 (7.6e-4 at 0.30, 3.2e-2 at 0.35) and to 0.35 fs_out at T = 64.
BAND = {(16_368_000, 8_184_000, 32): 0.25}


@pytest.mark.parametrize("fs_in,fs_out,taps", [(a, b, 32) for a, b in PAIRS] + [(16_368_000, 8_184_000, 64)])
def test_model_passes_tones_within_the_passband(fs_in, fs_out, taps):
    """A complex tone at |f| <= 0.35 min(fs_in, fs_out) comes through at the right instant with error <= 2e-4 of its amplitude."""
    band = BAND.get((fs_in, fs_out, taps), 0.35)
    n_ms = 3
    n_in = fs_in // 1000
    t_in = np.arange((n_ms + 2) * n_in) / fs_in
    t_out = np.arange(n_ms * (fs_out // 1000)) / fs_out
    edge = 80   # outputs whose taps reach before sample 0 see the zero padding
    for f in np.array([-1.0, -0.6, 0.0, 0.3, 1.0]) * band * min(fs_in, fs_out):
        x = np.exp(2j * np.pi * f * t_in + 0.3j)
        y = model.resample(x, fs_in, fs_out, 0, n_ms, taps)
        want = np.exp(2j * np.pi * f * t_out + 0.3j)
        assert np.abs(y - want)[edge:].max() <= 2e-4, f


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
