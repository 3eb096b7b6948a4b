"""The notch's host side (no GPU): gyp_tones_find and gyp_tone_refine against tests/notch_model.py on constructed spectra and
records, every argument rule of the tone lists, the record layouts, the ingest entry points on a handle without a context, and the
gate of the end-to-end scene: the oracle misses planted satellites under the CW and finds all four once the model has notched it."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import notch_model as model
from gypsum_amd import _lib
from gypsum_amd import notch as nt
from oracle import gypsum_oracle as orc

HEADER = Path(__file__).resolve().parents[1] / "include" / "gypsum_hip.h"
BAD = _lib.GYP_E_BAD_ARG


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------------------- gyp_tones_find
def _flat(n=64, level=1.0):
    return np.full(n, level)


def _spectra():
    rng = np.random.default_rng(7)
    out = {}
    p = _flat()
    p[[10, 30, 50]] = [40.0, 90.0, 20.0]
    out["three peaks, strongest first"] = (p, 8.0, 2, 8)
    p = _flat()
    p[[10, 30]] = 50.0
    out["a tie: the lowest bin first"] = (p, 8.0, 2, 8)
    p = _flat()
    p[20:24] = 50.0
    out["a plateau: its lowest bin"] = (p, 8.0, 1, 8)
    p = _flat()
    p[0], p[63] = 30.0, 60.0
    out["maxima at bin 0 and at the last bin"] = (p, 8.0, 2, 8)
    p = _flat()
    p[0:2], p[62:64] = 30.0, 60.0
    out["plateaus at both ends"] = (p, 8.0, 1, 8)
    p = _flat()
    p[[5, 40]] = [8.0, 7.999999999]
    out["threshold exactly met, and just missed"] = (p, 8.0, 2, 8)
    p = _flat()
    p[4:60:5] = 20.0 + np.arange(len(p[4:60:5]))
    out["more candidates than max_tones"] = (p, 8.0, 2, 3)
    p = _flat()
    p[[20, 22, 27]] = [50.0, 49.0, 30.0]
    out["separation drops the neighbour, keeps the next"] = (p, 8.0, 5, 8)
    out["separation exactly met"] = (p, 8.0, 7, 8)
    out["max_tones 0"] = (p, 8.0, 2, 0)
    out["noise, even count"] = (rng.exponential(1.0, 512), 4.0, 3, 8)
    out["noise, odd count"] = (rng.exponential(1.0, 511), 4.0, 3, 8)
    out["one bin"] = (np.array([3.0]), 1.0, 1, 8)
    out["all zero"] = (np.zeros(16), 2.0, 1, 8)
    return out


@pytest.mark.parametrize("name", list(_spectra()))
def test_tones_find_equals_the_model(lib, name):
    power, threshold, sep, max_tones = _spectra()[name]
    want = model.tones_find(power, threshold, sep, max_tones)
    assert nt.find_tones(power, 999.0, threshold, sep, max_tones) == want, name
    expected = {"three peaks, strongest first": [30, 10, 50], "a tie: the lowest bin first": [10, 30], "a plateau: its lowest bin": [20],
                "maxima at bin 0 and at the last bin": [63, 0], "plateaus at both ends": [62, 0],
                "threshold exactly met, and just missed": [5], "more candidates than max_tones": [59, 54, 49],
                "separation drops the neighbour, keeps the next": [20, 27], "separation exactly met": [20, 27], "max_tones 0": [],
                "one bin": [0], "all zero": []}
    if name in expected:
        assert want == expected[name], (name, want)
    else:
        assert 0 < len(want) <= max_tones


def test_tones_find_refuses_bad_arguments(lib):
    p = _flat(16)
    bins = np.zeros(8, dtype=np.int32)

    def refused(rc, what):
        msg = (lib.gyp_last_error(None) or b"").decode()
        assert rc == BAD and msg.startswith("gyp_tones_find"), (what, rc, msg)

    refused(lib.gyp_tones_find(None, 16, 1.0, 2.0, 1, 8, _lib.ptr(bins)), "power NULL")
    refused(lib.gyp_tones_find(_lib.ptr(p), 16, 1.0, 2.0, 1, 8, None), "out_bins NULL")
    refused(lib.gyp_tones_find(_lib.ptr(p), 0, 1.0, 2.0, 1, 8, _lib.ptr(bins)), "n_freq 0")
    refused(lib.gyp_tones_find(_lib.ptr(p), 16, 1.0, 2.0, 0, 8, _lib.ptr(bins)), "separation 0")
    refused(lib.gyp_tones_find(_lib.ptr(p), 16, 1.0, 2.0, 1, -1, _lib.ptr(bins)), "max_tones -1")
    for v in (0.0, -1.0, np.inf, np.nan):
        refused(lib.gyp_tones_find(_lib.ptr(p), 16, 1.0, v, 1, 8, _lib.ptr(bins)), f"threshold {v}")
        refused(lib.gyp_tones_find(_lib.ptr(p), 16, v, 2.0, 1, 8, _lib.ptr(bins)), f"freq_step_hz {v}")
    for v in (-1.0, np.inf, np.nan):
        q = p.copy()
        q[3] = v
        refused(lib.gyp_tones_find(_lib.ptr(q), 16, 1.0, 2.0, 1, 8, _lib.ptr(bins)), f"power {v}")
    with pytest.raises(_lib.GypsumHipError, match="gyp_tones_find"):
        nt.find_tones(p, 1.0, 0.0, 1)


# ---------------------------------------------------------------------------------------------------- gyp_tone_refine
@pytest.mark.parametrize("delta", [0.0, 0.4, -37.25, 480.0, -499.0])
def test_refine_equals_the_model_and_recovers_the_offset(lib, delta):
    """Records of a tone `delta` Hz off, block = 1 ms (valid for |delta| < 500 Hz), with a little noise."""
    rng = np.random.default_rng(int(abs(delta) * 4))
    t_b = 1e-3
    a = 3.0 * np.exp(2j * np.pi * delta * t_b * np.arange(12) + 0.3) + 0.003 * (rng.standard_normal(12) + 1j * rng.standard_normal(12))
    rec = np.zeros(12, dtype=nt.TONE_DTYPE)
    rec["re"], rec["im"] = a.real, a.imag
    got, want = nt.refine(rec, t_b), model.refine(a, t_b)
    assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (got, want)
    assert abs(got - delta) < 0.2
    assert nt.refine(rec[:2], t_b) == pytest.approx(model.refine(a[:2], t_b), abs=1e-9)


def test_refine_refuses_bad_arguments(lib):
    rec = np.zeros(4, dtype=nt.TONE_DTYPE)
    d = C.c_double(7.0)
    for what, rc in (("records NULL", lib.gyp_tone_refine(None, 4, 1e-3, C.byref(d))), ("out NULL", lib.gyp_tone_refine(_lib.ptr(rec), 4, 1e-3, None)),
                     ("one block", lib.gyp_tone_refine(_lib.ptr(rec), 1, 1e-3, C.byref(d))), ("seconds 0", lib.gyp_tone_refine(_lib.ptr(rec), 4, 0.0, C.byref(d))),
                     ("seconds nan", lib.gyp_tone_refine(_lib.ptr(rec), 4, np.nan, C.byref(d)))):
        assert rc == BAD and (lib.gyp_last_error(None) or b"").decode().startswith("gyp_tone_refine"), what
    assert d.value == 7.0
    assert lib.gyp_tone_refine(_lib.ptr(rec), 4, 1e-3, C.byref(d)) == 0 and d.value == 0.0      # all-zero records: no slope


# ---------------------------------------------------------------------------------------------------- argument rules
def test_tone_lists_are_checked_before_anything_is_launched(lib):
    """gyp_notch_iq_dev refuses a NULL context first; the rules themselves are checked through a handle without a context below and
    on the device in tests/test_gpu_notch.py; the Python mirror of the rules must agree with them."""
    fs = 2_046_000
    nt.check_tones([], fs)
    nt.check_tones([0, 4000, -4000, 8000, 12000, 16000, 20000, 24000], fs)
    nt.check_tones([fs // 2 - 1, -(fs // 2 - 1)], fs)
    for bad in ([0] * 9, list(range(0, 9 * 4000, 4000)), [100_000, 103_999], [fs // 2], [-(fs // 2)], [fs]):
        with pytest.raises(ValueError):
            nt.check_tones(bad, fs)
    nt.check_tones([100_000, 104_000], fs)
    rec = nt.notch_records([[1, 2], []])
    assert rec["count"].tolist() == [2, 0] and rec["freq_hz"][0, :2].tolist() == [1, 2]
    assert len(nt.notch_records([217_300], 3)) == 3
    with pytest.raises(ValueError):
        nt.notch_records([list(range(9))])
    one = np.zeros(1, dtype=nt.NOTCH_DTYPE)
    assert lib.gyp_notch_iq_dev(None, None, None, 1, 0, 0, 1, 2046, fs, _lib.ptr(one)) == BAD
    assert lib.gyp_iq_tones_dev(None, None, 1, 0, 0, 1, 64, fs, None, 1, 0, None) == BAD


def test_record_layouts_match_the_header(tmp_path):
    structs = {"gyp_tone_rec": _lib.TONE_REC, "gyp_notch_tones": _lib.NOTCH_TONES}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for name, dt in structs.items():
        lines.append(f'printf("{name} size %zu\\n", sizeof({name}));')
        for field in dt.names:
            lines.append(f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    lines.append('printf("max tones %d\\n", GYP_NOTCH_MAX_TONES);')
    lines.append('printf("windows rect_hann %d\\n", GYP_WINDOW_RECT * 10 + GYP_WINDOW_HANN);')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {(l.split()[0], l.split()[1]): int(l.split()[2]) for l in out}
    assert got[("gyp_tone_rec", "size")] == _lib.TONE_REC.itemsize == _lib.RECORD_SIZES["gyp_tone_rec"] == 16
    assert got[("gyp_notch_tones", "size")] == _lib.NOTCH_TONES.itemsize == _lib.RECORD_SIZES["gyp_notch_tones"] == 72
    for name, dt in structs.items():
        for field in dt.names:
            assert got[(name, field)] == dt.fields[field][1], (name, field)
    assert got[("max", "tones")] == _lib.GYP_NOTCH_MAX_TONES == 8 and got[("windows", "rect_hann")] == 1


def test_a_handle_without_a_context_has_no_notches(lib, tmp_path):
    path = tmp_path / "x.bin"
    np.zeros(2 * 2046 * 5, dtype=np.uint8).tofile(path)
    h = C.c_void_p()
    assert lib.gyp_ingest_open(None, str(path).encode(), _lib.GYP_FMT_U8, 2_046_000, 2046, 1, 3, C.byref(h)) == 0
    try:
        f = np.array([217_300], dtype=np.int64)
        out, n = np.zeros(8, dtype=np.int64), C.c_int32(7)
        for call, name in ((lambda: lib.gyp_ingest_set_notches(h, _lib.ptr(f), 1), "gyp_ingest_set_notches"),
                           (lambda: lib.gyp_ingest_set_notches(h, None, 0), "gyp_ingest_set_notches"),
                           (lambda: lib.gyp_ingest_get_notches(h, _lib.ptr(out), C.byref(n)), "gyp_ingest_get_notches"),
                           (lambda: lib.gyp_ingest_find_tones(h, 0, 2, 16.0, 8, 1, _lib.ptr(out), None, C.byref(n)), "gyp_ingest_find_tones")):
            assert call() == BAD and (lib.gyp_last_error(None) or b"").decode().startswith(name)
        assert n.value == 7 and not out.any()                 # nothing was written
        raw, first, n_ms = C.c_void_p(), C.c_int64(), C.c_int32()
        assert lib.gyp_ingest_next_host(h, C.byref(raw), C.byref(first), C.byref(n_ms)) == 0 and (first.value, n_ms.value) == (0, 1)
        assert lib.gyp_ingest_set_notches(None, None, 0) == BAD and lib.gyp_ingest_get_notches(None, None, None) == BAD
        assert lib.gyp_ingest_find_tones(None, 0, 2, 16.0, 8, 0, None, None, None) == BAD
    finally:
        lib.gyp_ingest_close(h)


# ---------------------------------------------------------------------------------------------------- the model itself
def test_the_model_removes_a_tone_and_leaves_the_rest():
    """An on-frequency tone goes to rounding level; 0.4 Hz off it is suppressed by > 50 dB; 50 Hz off by about 20 dB (documented);
    white noise loses 1 / N of its power per tone; an empty list returns the input."""
    fs, n = model.SCENE_FS, model.SCENE_N
    i = np.arange(4 * n)
    rng = np.random.default_rng(3)
    for off, lo, hi in ((0.0, 250.0, 400.0), (0.4, 50.0, 140.0), (50.0, 17.0, 23.0)):
        x = 5.0 * np.exp(1j * (2.0 * np.pi * (217_300 + off) / fs * i + 0.1))
        y, amps = model.notch(x, fs, n, [217_300])
        db = -10.0 * np.log10(np.mean(np.abs(y) ** 2) / 25.0)
        assert lo < db < hi, (off, db)
        assert np.allclose(np.abs(amps), 5.0, rtol=2e-2)
    noise = rng.standard_normal(4 * n) + 1j * rng.standard_normal(4 * n)
    y, _ = model.notch(noise, fs, n, [217_300, -400_000])
    assert np.mean(np.abs(y) ** 2) == pytest.approx(np.mean(np.abs(noise) ** 2) * (1 - 2.0 / n), rel=2e-3)
    assert np.array_equal(model.notch(noise, fs, n, [])[0], noise)
    # the phase is a function of the absolute index: a window starting at 2^40 + 17 equals the same indices of a longer stream
    big = 2 ** 40 + 17
    assert np.array_equal(model.phase_turns(217_300, big, 100, fs), model.phase_turns(217_300, big % fs, 100, fs))
    a = model.tones(x, fs, [217_300, 217_350], 64, model.HANN, first_index=0)
    assert a.shape == (4 * n // 64, 2) and np.allclose(np.abs(a[:, 1]), 5.0, rtol=1e-3)


# ---------------------------------------------------------------------------------------------------- the scene's gate
def test_the_scene_hides_planted_satellites_under_the_tone_and_the_model_notch_uncovers_all_four():
    """Un-notched the oracle's acquisition must miss at least one planted satellite; on the model-notched samples it must find all
    four at their planted code phases and Doppler (within 50 Hz: ten non-coherent milliseconds resolve the Doppler to a few tens of
    Hz in this noise, the search's own last step is 1 Hz) and above the detection threshold."""
    x, clean = model.scene(10)
    assert np.abs(x).max() > 90 * np.abs(clean).std() / np.sqrt(2)          # the tone is there: 100 sigma
    y, amps = model.notch(x, model.SCENE_FS, model.SCENE_N, [model.SCENE_TONE_HZ])
    chips = orc.generate_ca_codes()

    def found(data):
        ok = []
        for sv, (cp, doppler) in model.SCENE_SATS.items():
            o = orc.acquire_satellite(sv, np.asarray(data, dtype=np.complex128), model.SCENE_FS, model.SCENE_N,
                                      orc.prn_as_complex(chips[sv - 1], model.SCENE_N))
            print(f"PRN {sv}: Doppler {o.doppler_shift} code phase {o.prn_phase_shift} strength {o.correlation_strength:.2f}; planted {doppler} {cp}")
            ok.append(o.prn_phase_shift == cp and abs(o.doppler_shift - doppler) <= 50 and
                      o.correlation_strength > orc.ACQUISITION_STRENGTH_THRESHOLD)
        return ok

    assert not all(found(x))
    assert all(found(y))
