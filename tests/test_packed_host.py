"""Packed recordings on the host (no GPU): the numpy model against hand-worked bytes, gypsum_amd.packing.pack and the presets'
formulas; gyp_packed_span against the model; the gyp_packing layout against its ctypes mirror; every validation error."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import packed_model as model
from gypsum_amd import _lib, synth
from gypsum_amd import packing as pk

HEADER = Path(__file__).resolve().parents[1] / "include" / "gypsum_hip.h"
PRESETS = ("sign_magnitude", "twos_complement", "offset_binary")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_hand_worked_bytes_pin_each_bit_order():
    b = bytes([0b00_01_10_11])
    assert list(model.unpack_codes(b, 2, "msb")) == [0, 1, 2, 3]
    assert list(model.unpack_codes(b, 2, "lsb")) == [3, 2, 1, 0]
    sm = pk.sign_magnitude(2)
    assert list(np.asarray(sm.levels)[model.unpack_codes(b, 2, "msb")]) == [1, 3, -1, -3]
    assert list(model.unpack_codes(bytes([0b1000_0001]), 1, "msb")) == [1, 0, 0, 0, 0, 0, 0, 1]
    assert list(model.unpack_codes(bytes([0b1100_0000]), 1, "lsb")) == [0, 0, 0, 0, 0, 0, 1, 1]
    assert list(model.unpack_codes(bytes([0x1f]), 4, "msb")) == [1, 15]
    assert list(model.unpack_codes(bytes([0x1f]), 4, "lsb")) == [15, 1]
    assert pk.pack([0, 1, 2, 3], pk.sign_magnitude(2)) == b
    assert pk.pack([0, 1, 2, 3], pk.sign_magnitude(2, order="lsb")) == bytes([0b11_10_01_00])


def test_preset_formulas():
    assert pk.sign_magnitude(1).levels == (1, -1)
    assert pk.sign_magnitude(2).levels == (1, 3, -1, -3)
    assert pk.sign_magnitude(4).levels == tuple(range(1, 16, 2)) + tuple(-x for x in range(1, 16, 2))
    assert pk.twos_complement(2).levels == (0, 1, -2, -1)
    assert pk.twos_complement(4).levels == tuple(range(8)) + tuple(range(-8, 0))
    assert pk.offset_binary(2).levels == (-3, -1, 1, 3)
    assert pk.offset_binary(1).levels == (-1, 1)
    for name in PRESETS:
        for bits in (1, 2, 4):
            lv = np.asarray(pk.PRESETS[name](bits).levels)
            assert np.array_equal(lv, np.rint(lv)) and np.abs(lv).max() <= 15


@pytest.mark.parametrize("bits", [1, 2, 4])
@pytest.mark.parametrize("order", ["msb", "lsb"])
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("real", [False, True])
def test_pack_round_trips_through_the_model(bits, order, preset, real):
    p = pk.PRESETS[preset](bits, real=real, order=order)
    rng = np.random.default_rng([bits, len(order), len(preset), real])
    for n in (0, 1, 7, 8, 9, 1001):
        codes = rng.integers(0, 1 << bits, n)
        data = pk.pack(codes, p)
        assert len(data) == -(-n * bits // 8)
        assert np.array_equal(model.unpack_codes(data, bits, order, n), codes)
    # quantize picks the level's own code, and the values follow levels[code] * scale
    x = np.asarray(p.levels, dtype=np.float64) * 0.25
    assert np.array_equal(pk.quantize(x, p, 0.25), np.arange(1 << bits)) or len(set(p.levels)) < len(p.levels)


def _span(lib, p, spm, file_bytes, first, n):
    outs = [C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()]
    rec = p.record()
    rc = lib.gyp_packed_span(_lib.ptr(rec), spm, file_bytes, first, n, *[C.byref(o) for o in outs])
    assert rc == 0, lib.gyp_last_error(None)
    keys = ("in_first", "in_n", "first_byte", "bit0", "n_bytes", "file_samples", "total_ms")
    return dict(zip(keys, (o.value for o in outs)))


@pytest.mark.parametrize("bits", [1, 2, 4])
@pytest.mark.parametrize("real", [False, True])
def test_span_matches_the_model(lib, bits, real):
    p = pk.sign_magnitude(bits, real=real)
    rng = np.random.default_rng([bits, real])
    for k in (1, 3, 5):
        n_in = 1023 * k
        B = p.sample_bits
        for _ in range(40):
            file_samples = int(rng.integers(0, 9 * n_in))
            extra_bits = int(rng.integers(0, B)) if rng.random() < 0.5 else 0       # a trailing partial sample
            file_bytes = (file_samples * B + extra_bits + 7) // 8
            ms = int(rng.integers(0, 8))
            halo = int(rng.integers(0, 64))
            first, n = ms * n_in - halo, int(rng.integers(1, 3)) * n_in + 2 * halo
            got = _span(lib, p, n_in, file_bytes, first, n)
            assert got == model.span(bits, real, file_bytes, first, n, n_in), (k, file_bytes, first, n)
        # millisecond edges mid-byte: 2-bit I,Q at K = 1, 3, 5 is 511.5 K bytes a millisecond
        got = _span(lib, p, n_in, 10 * n_in * B // 8 + 1, n_in, n_in)
        assert got["bit0"] == (n_in * B) % 8
        assert got["total_ms"] == (got["file_samples"] - 1) // n_in


def test_total_ms_equals_the_int8_twins(lib, tmp_path):
    """total_ms counted in samples equals gyp_ingest_open's (size - 1) / ms_bytes on the int8 I,Q file of the same words."""
    p = pk.sign_magnitude(2)
    for file_bytes in (1, 1022, 1023, 1024, 2046, 2047, 10 * 1023):
        got = _span(lib, p, 2046, file_bytes, 0, 0)
        file_samples = got["file_samples"]
        assert file_samples == 2 * file_bytes
        twin = tmp_path / "twin.bin"
        twin.write_bytes(bytes(2 * file_samples))
        h = C.c_void_p()
        assert lib.gyp_ingest_open(None, str(twin).encode(), _lib.GYP_FMT_I8, 2_046_000, 2046, 1, 3, C.byref(h)) == 0
        assert lib.gyp_ingest_total_ms(h) == got["total_ms"]
        lib.gyp_ingest_close(h)


def test_packing_layout_matches_the_header(tmp_path):
    dt = _lib.PACKING
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(gyp_packing));']
    for field in dt.names:
        lines.append(f'printf("{field} %zu\\n", offsetof(gyp_packing, {field}));')
    lines.append('printf("MSB %d LSB %d\\n", GYP_PACK_MSB_FIRST, GYP_PACK_LSB_FIRST);')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {l.split()[0]: int(l.split()[1]) for l in out[:-1]}
    assert got["size"] == dt.itemsize == _lib.RECORD_SIZES["gyp_packing"] == 80
    for field in dt.names:
        assert got[field] == dt.fields[field][1], field
    assert out[-1] == f"MSB {_lib.GYP_PACK_MSB_FIRST} LSB {_lib.GYP_PACK_LSB_FIRST}"


def _bad_records():
    base = pk.sign_magnitude(2).record()
    cases = {}
    for bits in (0, 3, 8, -1):
        r = base.copy()
        r["bits"] = bits
        cases[f"bits={bits}"] = r
    r = base.copy()
    r["reserved"] = 1
    cases["reserved"] = r
    r = base.copy()
    r["order"] = 2
    cases["order"] = r
    r = base.copy()
    r["real"] = 2
    cases["real=2"] = r
    for v in (np.nan, np.inf):
        r = base.copy()
        r["levels"][0, 3] = v
        cases[f"level {v}"] = r
    return cases


def test_every_validation_error(lib, tmp_path):
    o = C.c_int64()
    for what, rec in _bad_records().items():
        assert lib.gyp_packed_span(_lib.ptr(rec), 2046, 100, 0, 10, None, None, None, None, None, None, None) == _lib.GYP_E_BAD_ARG, what
        h = C.c_void_p()
        assert lib.gyp_ingest_open_packed(None, b"/nonexistent", _lib.ptr(rec), 2_046_000, 0, 0, 10, 4, C.byref(h)) == _lib.GYP_E_BAD_ARG
    assert lib.gyp_packed_span(None, 2046, 100, 0, 10, None, None, None, None, None, None, None) == _lib.GYP_E_BAD_ARG
    # a level past 2^bits is ignored, even if it is not finite
    rec = pk.sign_magnitude(2).record()
    rec["levels"][0, 4] = np.nan
    assert lib.gyp_packed_span(_lib.ptr(rec), 2046, 100, 0, 10, None, None, None, None, None, None, C.byref(o)) == 0
    good = pk.sign_magnitude(2).record()
    for spm, fb, n in ((0, 100, 10), (2046, -1, 10), (2046, 100, -1)):
        assert lib.gyp_packed_span(_lib.ptr(good), spm, fb, 0, n, None, None, None, None, None, None, None) == _lib.GYP_E_BAD_ARG
    # the device entries refuse a NULL context; the ingest needs one
    assert lib.gyp_unpack_iq_dev(None, _lib.ptr(good), None, 1, 16, 0, 4, 1.0, 4, None) == _lib.GYP_E_BAD_ARG
    assert lib.gyp_resample_packed_dev(None, _lib.ptr(good), None, 1, 16, 0, 0, 4, 1.0, 2_048_000, 0, 0, 0, 1, 2046, None) == _lib.GYP_E_BAD_ARG
    h = C.c_void_p()
    assert lib.gyp_ingest_open_packed(None, b"/nonexistent", _lib.ptr(good), 2_046_000, 0, 0, 10, 4, C.byref(h)) == _lib.GYP_E_BAD_ARG
    assert lib.gyp_ingest_open_packed(None, b"/nonexistent", _lib.ptr(good), 2_046_000, 0, 0, 10, 4, None) == _lib.GYP_E_BAD_ARG


def test_python_argument_errors(tmp_path):
    with pytest.raises(ValueError):
        pk.Packing(3, tuple(range(8)))
    with pytest.raises(ValueError):
        pk.Packing(2, (1, 2, 3))
    with pytest.raises(ValueError):
        pk.Packing(2, (1, 2, 3, np.nan))
    with pytest.raises(ValueError):
        pk.Packing(2, (1, 2, 3, 4), order="big")
    with pytest.raises(ValueError):
        pk.pack([4], pk.sign_magnitude(2))
    with pytest.raises(ValueError):
        pk.quantize(np.ones(3, dtype=complex), pk.sign_magnitude(2, real=True))
    from gypsum_amd.ingest import IqFileIngest
    from gypsum_amd.radio_input import InputFileInfo
    with pytest.raises(ValueError, match="leave sample_component_data_type out"):
        IqFileIngest(tmp_path / "x", 2_046_000, np.int8, packing=pk.sign_magnitude(2))
    with pytest.raises(ValueError, match="engine"):
        IqFileIngest(tmp_path / "x", 2_046_000, packing=pk.sign_magnitude(2))
    with pytest.raises(ValueError):
        InputFileInfo.packed(tmp_path / "x", 16_368_000, pk.sign_magnitude(2, real=True))
    with pytest.raises(ValueError):
        InputFileInfo.packed(tmp_path / "x", 2_046_000, pk.sign_magnitude(2), if_hz=4_092_000)
    info = InputFileInfo.packed(tmp_path / "x", 16_368_000, pk.sign_magnitude(2, real=True), if_hz=4_092_000)
    assert info.packing.real and info.if_hz == 4_092_000 and info.sample_component_data_type is np.uint8
    with pytest.raises(ValueError):
        synth.write_packed(np.ones(4), pk.sign_magnitude(2, real=True), tmp_path / "y", tail_words=1)


def test_write_packed_twin_holds_the_levels(tmp_path):
    rng = np.random.default_rng(5)
    for p in (pk.sign_magnitude(2), pk.offset_binary(1, real=True), pk.twos_complement(4, order="lsb")):
        x = rng.standard_normal(1001) + (1j * rng.standard_normal(1001) if not p.real else 0)
        tail = 1 if not p.real else 0
        info = synth.write_packed(x, p, tmp_path / "p.bin", tmp_path / "t.bin", tail_words=tail)
        data = (tmp_path / "p.bin").read_bytes()
        twin = np.fromfile(tmp_path / "t.bin", dtype=np.int8)
        assert twin.size == info["file_samples"] * p.words_per_sample
        vals = model.unpack_values(data, p.bits, p.order, p.levels, p.real)
        words = vals.view(np.float32) if not p.real else vals
        assert np.array_equal(words, twin.astype(np.float32))
