"""The down-converter's host side (no GPU): the library's design against the float64 model of the contract, the automatic tap
count, the rate rule at its boundaries, the model's passband per T * ratio, and the rate helpers."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from gypsum_amd import _lib
from gypsum_amd import resample as rs

import ddc_model as model

# (fs_in, fs_out, if_hz): the front ends the contract names
PAIRS = [(16_368_000, 4_092_000, 4_092_000), (16_368_000, 8_184_000, 4_092_000), (16_368_000, 4_092_000, -4_092_000),
         (38_192_000, 8_184_000, 9_548_000), (38_192_000, 16_368_000, 9_548_000), (5_000_000, 2_046_000, 1_250_000)]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _ulp32(v: np.ndarray) -> np.ndarray:
    _, e = np.frexp(np.abs(v))
    return np.ldexp(1.0, e - 24)


@pytest.mark.parametrize("taps", model.TAPS)
@pytest.mark.parametrize("fs_in,fs_out,if_hz", PAIRS)
def test_design_is_the_float64_model_rounded_to_float32(fs_in, fs_out, if_hz, taps):
    got = rs.ddc_design(fs_in, fs_out, if_hz, taps)
    want = model.design(fs_in, fs_out, taps)
    assert got.shape == want.shape == (model.resample_model.n_phases(fs_in, fs_out), taps)
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= 0.5 * _ulp32(want) + 1e-9 * np.abs(want))
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6


@pytest.mark.parametrize("fs_in,fs_out,if_hz", PAIRS)
def test_design_is_the_resamplers_at_the_same_rates_and_taps(fs_in, fs_out, if_hz):
    """Same windowed sinc, same fc = 0.9 fs_out / fs_in: the two host entry points agree bit for bit where both are defined."""
    if 2 * fs_out >= fs_in:
        assert rs.ddc_design(fs_in, fs_out, if_hz, 32).tobytes() == rs.design(fs_in, fs_out, 32).tobytes()


def test_auto_taps(lib):
    L, t = C.c_int32(), C.c_int32()
    for fs_in, fs_out, if_hz, want in ((16_368_000, 4_092_000, 4_092_000, 64), (38_192_000, 8_184_000, 9_548_000, 96),
                                       (16_368_000, 8_184_000, 4_092_000, 32), (38_192_000, 16_368_000, 9_548_000, 48),
                                       (5_000_000, 2_046_000, 1_250_000, 48), (32_736_000, 4_092_000, 8_184_000, 128),
                                       (24_552_000, 4_092_000, 6_138_000, 96)):
        assert lib.gyp_ddc_design(fs_in, fs_out, if_hz, 0, None, C.byref(L), C.byref(t)) == _lib.GYP_OK
        assert t.value == want == model.resolve_taps(fs_in, fs_out), (fs_in, fs_out)
        assert t.value * fs_out >= 16 * fs_in
        assert L.value == model.resample_model.n_phases(fs_in, fs_out)
        assert rs.ddc_design(fs_in, fs_out, if_hz, 0).tobytes() == rs.ddc_design(fs_in, fs_out, if_hz, want).tobytes()
    for fs_in, fs_out, if_hz, taps in ((16_368_000, 4_092_000, 4_092_000, 32), (16_368_000, 4_092_000, 4_092_000, 128)):
        assert lib.gyp_ddc_design(fs_in, fs_out, if_hz, taps, None, None, C.byref(t)) == _lib.GYP_OK and t.value == taps


def _code(lib, fs_in, fs_out, if_hz, taps=0):
    return lib.gyp_ddc_design(fs_in, fs_out, if_hz, taps, None, None, None)


def test_rule_boundaries(lib):
    """Accepted or refused exactly at the inequalities, for both signs of if_hz."""
    fs_out = 4_092_000
    # 20 |if| >= 9 fs_out: |if| >= 1_841_400
    fs_in = 16_368_000
    for sign in (1, -1):
        assert _code(lib, fs_in, fs_out, sign * 1_841_400) == _lib.GYP_OK
        assert _code(lib, fs_in, fs_out, sign * 1_841_399) == _lib.GYP_E_BAD_RATE
        # 20 |if| + 9 fs_out <= 10 fs_in: |if| <= (163_680_000 - 36_828_000) / 20 = 6_342_600
        assert _code(lib, fs_in, fs_out, sign * 6_342_600) == _lib.GYP_OK
        assert _code(lib, fs_in, fs_out, sign * 6_342_601) == _lib.GYP_E_BAD_RATE
    assert _code(lib, fs_in, fs_out, 0) == _lib.GYP_E_BAD_RATE
    # 8 fs_out >= fs_in: 32.736 Msps is the last input rate for 4.092 Msps out
    assert _code(lib, 32_736_000, fs_out, 8_184_000) == _lib.GYP_OK
    assert _code(lib, 32_737_000, fs_out, 8_184_000) == _lib.GYP_E_BAD_RATE
    # fs_out / fs_in <= 5/9 exactly: 9 fs_out = 5 fs_in, |if| = fs_in / 4
    assert _code(lib, 9_000_000, 5_000_000, 2_250_000) == _lib.GYP_OK
    assert _code(lib, 9_000_000, 5_001_000, 2_250_000) == _lib.GYP_E_BAD_RATE
    assert _code(lib, 9_000_000, 5_000_000, -2_250_000) == _lib.GYP_OK
    for a, b, f in ((16_368_500, 4_092_000, 4_092_000), (16_368_000, 4_092_500, 4_092_000), (0, 4_092_000, 4_092_000),
                    (-16_368_000, 4_092_000, 4_092_000), (16_368_000, 0, 4_092_000), (16_368_000, 16_368_000, 4_092_000),
                    (16_368_000, 4_092_000, 2 ** 62), (16_368_000, 4_092_000, -2 ** 63), (2 ** 31 * 1000, 300_000_000_000, 10 ** 11)):
        assert _code(lib, a, b, f) == _lib.GYP_E_BAD_RATE, (a, b, f)
    for t in (-1, 16, 24, 31, 33, 80, 256):
        assert _code(lib, 16_368_000, 4_092_000, 4_092_000, t) == _lib.GYP_E_BAD_ARG, t
    # a grid of rates and IFs against the model's rule
    for fs_in in (4_000_000, 16_368_000, 38_192_000):
        for fs_out in (1_023_000, 2_046_000, 4_092_000, 8_184_000, 16_368_000):
            for if_hz in (-9_548_000, -4_092_000, -1_000_000, 1_000_000, 1_250_000, 4_092_000, 9_548_000, 4_130_400):
                want = _lib.GYP_OK if model.rates_ok(fs_in, fs_out, if_hz) else _lib.GYP_E_BAD_RATE
                assert _code(lib, fs_in, fs_out, if_hz) == want, (fs_in, fs_out, if_hz)
    with pytest.raises(_lib.GypsumHipError) as e:
        rs.ddc_design(16_368_000, 4_092_000, 0)
    assert e.value.code == _lib.GYP_E_BAD_RATE


# The passband table of include/gypsum_hip.h: T * ratio -> B (fraction of fs_out), with the (fs_in, fs_out, if_hz, T) it is
# measured at (ratios 1/8, 1/4 and 1/2).
BAND = {6: (0.02, [(32_736_000, 4_092_000, 8_184_000, 48)]),
        8: (0.12, [(16_368_000, 4_092_000, 4_092_000, 32), (32_736_000, 4_092_000, 8_184_000, 64)]),
        12: (0.23, [(16_368_000, 4_092_000, 4_092_000, 48), (32_736_000, 4_092_000, 8_184_000, 96)]),
        16: (0.29, [(16_368_000, 4_092_000, 4_092_000, 64), (16_368_000, 8_184_000, 4_092_000, 32),
                    (32_736_000, 4_092_000, 8_184_000, 128)]),
        24: (0.34, [(16_368_000, 4_092_000, 4_092_000, 96), (16_368_000, 8_184_000, 4_092_000, 48)]),
        32: (0.37, [(16_368_000, 4_092_000, 4_092_000, 128), (16_368_000, 8_184_000, 4_092_000, 64)])}


def _tone_error(fs_in, fs_out, if_hz, taps, band):
    """max |y - (A/2) exp(j (2 pi d t + phi))| / (A/2) over tones at d = (-1, -0.6, 0, 0.3, 1) * band * fs_out."""
    n_ms = 2
    t_in = np.arange((n_ms + 1) * (fs_in // 1000)) / fs_in
    t_out = np.arange(n_ms * (fs_out // 1000)) / fs_out
    edge = 40   # outputs whose taps reach before sample 0 see the zero padding
    worst = 0.0
    for d in np.array([-1.0, -0.6, 0.0, 0.3, 1.0]) * band * fs_out:
        x = np.cos(2 * np.pi * (if_hz + d) * t_in + 0.3)
        y = model.ddc(x, fs_in, fs_out, if_hz, 0, n_ms, taps)
        want = 0.5 * np.exp(1j * (2 * np.pi * d * t_out + 0.3))
        worst = max(worst, np.abs(y - want)[edge:].max() / 0.5)
    return worst


@pytest.mark.parametrize("fs_in,fs_out,if_hz,taps,band", [(*c, b) for tr, (b, cs) in BAND.items() for c in cs])
def test_model_passes_tones_within_the_passband(fs_in, fs_out, if_hz, taps, band):
    assert taps * fs_out // fs_in in BAND
    assert _tone_error(fs_in, fs_out, if_hz, taps, band) <= 2e-4
    assert _tone_error(fs_in, fs_out, -if_hz, taps, band) <= 2e-4


def test_output_rates():
    assert rs.ddc_output_rates(16_368_000, 4_092_000) == (2_046_000, 3_069_000, 4_092_000, 5_115_000, 6_138_000, 8_184_000)
    assert rs.ddc_output_rates(16_368_000, -4_092_000) == rs.ddc_output_rates(16_368_000, 4_092_000)
    assert rs.default_ddc_rate(16_368_000, 4_092_000) == 8_184_000
    assert rs.ddc_output_rates(38_192_000, 9_548_000) == (5_115_000, 6_138_000, 8_184_000, 10_230_000, 12_276_000, 16_368_000, 20_460_000)
    assert rs.default_ddc_rate(38_192_000, 9_548_000) == 8_184_000
    assert rs.default_ddc_rate(5_000_000, 1_250_000) == 2_046_000
    # nothing at or below 8.184 Msps admitted: the smallest admitted one
    assert rs.ddc_output_rates(80_000_000, 20_000_000)[0] == 10_230_000
    assert rs.default_ddc_rate(80_000_000, 20_000_000) == 10_230_000
    for fs_in, if_hz in ((16_368_000, 0), (16_368_000, 8_184_000), (1_000_000, 250_000)):
        assert rs.ddc_output_rates(fs_in, if_hz) == ()
        with pytest.raises(ValueError):
            rs.default_ddc_rate(fs_in, if_hz)
    for fs_in, if_hz in ((16_368_000, 4_092_000), (38_192_000, -9_548_000), (80_000_000, 20_000_000)):
        for fs in rs.ddc_output_rates(fs_in, if_hz):
            assert model.rates_ok(fs_in, fs, if_hz)
            rs.ddc_design(fs_in, fs, if_hz)   # the library admits every rate the helper lists


def test_real_if_input_file_info(tmp_path):
    from gypsum_amd.radio_input import InputFileInfo, InputFileType
    info = InputFileInfo.real_if(tmp_path / "cap.bin", 16_368_000, 4_092_000)
    assert info.format is InputFileType.Raw and info.sdr_sample_rate == 16_368_000 and info.if_hz == 4_092_000
    assert np.dtype(info.sample_component_data_type) == np.int8
    info = InputFileInfo.real_if(tmp_path / "cap.bin", 38_192_000, -9_548_000, np.int16)
    assert info.if_hz == -9_548_000 and np.dtype(info.sample_component_data_type) == np.int16
    assert InputFileInfo.raw(tmp_path / "cap.bin", 4_000_000, np.int16).if_hz is None
    with pytest.raises(ValueError):
        InputFileInfo.real_if(tmp_path / "cap.bin", 16_368_000, 4_092_000, np.int32)


def test_render_real_if_is_twice_the_real_part_of_the_shifted_model():
    """x = 2 Re{s(t) exp(j 2 pi if_hz t)} with s render_at_rate's noiseless model (the IF phase reduced exactly), and real noise
    of sigma sqrt(2) * noise_sigma."""
    from gypsum_amd import synth
    scene = synth.random_scene(4_092_000, 3, 2, 5, noise_sigma=0.0)
    fs = 16_368_000
    s = synth.render_at_rate(scene, fs).astype(np.complex128)    # complex64: rounded to 2^-24 relative
    n = np.arange(len(s), dtype=np.int64)
    for if_hz in (4_092_000, -4_092_000, 4_130_400):
        x = synth.render_real_if(scene, fs, if_hz)
        assert x.dtype == np.float64 and len(x) == 3 * 16_368
        want = 2 * (s * np.exp(2j * np.pi * ((n * (if_hz % fs)) % fs) / fs)).real
        assert np.abs(x - want).max() <= 1e-6 * np.abs(s).max()
    noisy = synth.random_scene(4_092_000, 40, 1, 6, noise_sigma=0.5)
    noisy.sats.clear()
    x = synth.render_real_if(noisy, fs, 4_092_000)
    assert abs(x.std() / (np.sqrt(2) * 0.5) - 1) < 0.01
