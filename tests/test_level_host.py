"""The level's host side (no GPU): gyp_iq_level_from_stats against a Python float64 restatement of the header's order, bit for bit;
every error it must report; the layouts of gyp_iq_stats / gyp_iq_level against their numpy mirrors; and the ingest entry points on a
handle without a context."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import level_model as model
from gypsum_amd import _lib
from gypsum_amd import level as lv

HEADER = Path(__file__).resolve().parents[1] / "include" / "gypsum_hip.h"
BAD = _lib.GYP_E_BAD_ARG


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, stats, n_ms, n, remove_dc, target, want_measured=True):
    level = np.zeros(1, dtype=_lib.IQ_LEVEL)
    measured = np.full(4, np.nan)
    rc = lib.gyp_iq_level_from_stats(_lib.ptr(stats), n_ms, n, remove_dc, target, _lib.ptr(level), _lib.ptr(measured) if want_measured else None)
    return rc, level, measured


def _inputs():
    """(name, records, samples per ms) for n_ms = 100: numpy's exact statistics of uint8 words around 128, int8 and int16 words, and
    random float64 records."""
    rng = np.random.default_rng(209)
    n, n_ms = 2046, 100
    w8 = np.clip(np.rint(rng.normal(0.0, 14.0, n_ms * 2 * n)), -127, 127).astype(np.int8)
    u8 = (w8.astype(np.int16) + 128).astype(np.uint8)
    w16 = np.clip(np.rint(rng.normal(37.0, 900.0, n_ms * 2 * n)), -32767, 32767).astype(np.int16)
    out = [("uint8", model.stats_of_words(u8, n, 255.0), n), ("int8", model.stats_of_words(w8, n, 127.0), n),
           ("int16", model.stats_of_words(w16, n, 30000.0), n)]
    n = 8184
    r = np.zeros(n_ms, dtype=_lib.IQ_STATS)
    r["sum_re"] = rng.normal(0.3, 1.0, n_ms) * n
    r["sum_im"] = rng.normal(-0.1, 1.0, n_ms) * n
    r["sum_sq"] = (2.0 + rng.random(n_ms)) * n * 3.0
    r["max_abs"] = 5.0 + rng.random(n_ms)
    r["n_clip"] = rng.integers(0, 40, n_ms)
    out.append(("float64", r, n))
    return out


@pytest.mark.parametrize("remove_dc", [0, 1])
@pytest.mark.parametrize("n_ms", [1, 3, 100])
def test_level_from_stats_equals_the_float64_model_bit_for_bit(lib, n_ms, remove_dc):
    for name, stats, n in _inputs():
        st = np.ascontiguousarray(stats[:n_ms])
        for target in (1.0, 0.07, float(np.sqrt(2.0 / n))):
            rc, level, measured = _call(lib, st, n_ms, n, remove_dc, target)
            assert rc == 0, (name, (lib.gyp_last_error(None) or b"").decode())
            want_level, want_measured = model.level_from_stats(st, n, bool(remove_dc), target)
            got = np.array([level["dc_re"][0], level["dc_im"][0], level["gain"][0]], dtype=np.float32)
            assert np.array_equal(got.view(np.uint32), want_level.view(np.uint32)), (name, target, got, want_level)
            assert np.array_equal(measured.view(np.uint64), want_measured.view(np.uint64)), (name, target, measured, want_measured)
            assert level["reserved"][0] == 0
            if not remove_dc:
                assert level["dc_re"][0] == 0 and level["dc_im"][0] == 0
            # the Python wrapper returns the same numbers, and NULL for measured_out4 is allowed
            py_level, py_measured = lv.level_from_stats(st, n, target, remove_dc=bool(remove_dc))
            assert np.array_equal(np.array([py_level.dc_re, py_level.dc_im, py_level.gain], dtype=np.float32).view(np.uint32), got.view(np.uint32))
            assert [py_measured[k] for k in ("mean_re", "mean_im", "rms", "clipped")] == list(measured)
            rc2, level2, _ = _call(lib, st, n_ms, n, remove_dc, target, want_measured=False)
            assert rc2 == 0 and level2.tobytes() == level.tobytes()


def test_the_uint8_statistics_say_what_the_recording_is(lib):
    """Offset 128 is found to within the noise of the mean, and the gain brings the words' RMS about it to the target."""
    name, stats, n = _inputs()[0]
    level, measured = lv.level_from_stats(stats, n, 0.05)
    assert abs(level.dc_re - 128.0) < 0.1 and abs(level.dc_im - 128.0) < 0.1
    assert abs(measured["rms"] - 14.0 * np.sqrt(2.0)) < 0.2
    assert abs(level.gain * measured["rms"] - 0.05) < 1e-8
    assert measured["clipped"] == stats["n_clip"].sum() / (2.0 * len(stats) * n)


def test_every_error_case_returns_bad_arg_with_a_message(lib):
    _, stats, n = _inputs()[1]
    st = np.ascontiguousarray(stats[:3])
    level = np.zeros(1, dtype=_lib.IQ_LEVEL)

    def refused(rc, what):
        msg = (lib.gyp_last_error(None) or b"").decode()
        assert rc == BAD and msg.startswith("gyp_iq_level_from_stats"), (what, rc, msg)

    refused(lib.gyp_iq_level_from_stats(None, 3, n, 1, 1.0, _lib.ptr(level), None), "stats NULL")
    refused(lib.gyp_iq_level_from_stats(_lib.ptr(st), 3, n, 1, 1.0, None, None), "level_out NULL")
    refused(_call(lib, st, 0, n, 1, 1.0)[0], "n_ms 0")
    refused(_call(lib, st, -1, n, 1, 1.0)[0], "n_ms -1")
    refused(_call(lib, st, 3, 0, 1, 1.0)[0], "samples_per_ms 0")
    for target in (0.0, -1.0, np.inf, -np.inf, np.nan):
        refused(_call(lib, st, 3, n, 1, target)[0], f"target_rms {target}")
    # a constant recording: sum_sq / M == |mean|^2 exactly, so V = 0 with remove_dc = 1 ...
    const = model.stats_of_words(np.tile(np.array([128, 128], dtype=np.uint8), 3 * n), n)
    refused(_call(lib, const, 3, n, 1, 1.0)[0], "constant recording")
    # ... while without the offset's removal it has the power of its offset
    rc, lvl, _ = _call(lib, const, 3, n, 0, 1.0)
    assert rc == 0 and lvl["gain"][0] == np.float32(1.0 / np.sqrt(2 * 128.0 ** 2))
    # all-zero records (V = 0 either way), negative power (V < 0) and non-finite sums (V not finite)
    zero = np.zeros(3, dtype=_lib.IQ_STATS)
    for dc in (0, 1):
        refused(_call(lib, zero, 3, n, dc, 1.0)[0], "zero power")
    neg = st.copy()
    neg["sum_sq"] = -1.0
    refused(_call(lib, neg, 3, n, 0, 1.0)[0], "negative power")
    for v in (np.inf, np.nan):
        bad = st.copy()
        bad["sum_sq"][1] = v
        refused(_call(lib, bad, 3, n, 0, 1.0)[0], f"sum_sq {v}")
        bad = st.copy()
        bad["sum_re"][2] = v
        refused(_call(lib, bad, 3, n, 1, 1.0)[0], f"sum_re {v}")
    with pytest.raises(_lib.GypsumHipError, match="constant recording"):
        lv.level_from_stats(const, n, 1.0)


def test_record_layouts_match_the_header(tmp_path):
    structs = {"gyp_iq_stats": _lib.IQ_STATS, "gyp_iq_level": _lib.IQ_LEVEL}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for name, dt in structs.items():
        lines.append(f'printf("{name} size %zu\\n", sizeof({name}));')
        for field in dt.names:
            lines.append(f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    lines.append('printf("version version %d\\n", GYP_VERSION);')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {(l.split()[0], l.split()[1]): int(l.split()[2]) for l in out}
    assert got[("gyp_iq_stats", "size")] == _lib.IQ_STATS.itemsize == _lib.RECORD_SIZES["gyp_iq_stats"] == lv.STATS_DTYPE.itemsize == 32
    assert got[("gyp_iq_level", "size")] == _lib.IQ_LEVEL.itemsize == _lib.RECORD_SIZES["gyp_iq_level"] == 16
    for name, dt in structs.items():
        for field in dt.names:
            assert got[(name, field)] == dt.fields[field][1], (name, field)
    assert got[("version", "version")] == _lib.GYP_VERSION == 209


def test_a_handle_without_a_context_has_no_level(lib, tmp_path):
    path = tmp_path / "x.bin"
    np.zeros(2 * 2046 * 5, dtype=np.uint8).tofile(path)
    h = C.c_void_p()
    assert lib.gyp_ingest_open(None, str(path).encode(), _lib.GYP_FMT_U8, 2_046_000, 2046, 1, 3, C.byref(h)) == 0
    try:
        level = lv.IqLevel(128.0, 128.0, 0.01).record()
        out, on = np.zeros(1, dtype=_lib.IQ_LEVEL), C.c_int32(7)
        for name, rc in (("gyp_ingest_set_level", lib.gyp_ingest_set_level(h, _lib.ptr(level))),
                         ("gyp_ingest_set_level", lib.gyp_ingest_set_level(h, None)),
                         ("gyp_ingest_get_level", lib.gyp_ingest_get_level(h, _lib.ptr(out), C.byref(on))),
                         ("gyp_ingest_calibrate", lib.gyp_ingest_calibrate(h, 0, 2, 1, 1.0, 0.0, _lib.ptr(out), None))):
            assert rc == BAD, name
        for call, name in ((lambda: lib.gyp_ingest_set_level(h, _lib.ptr(level)), "gyp_ingest_set_level"),
                           (lambda: lib.gyp_ingest_get_level(h, _lib.ptr(out), C.byref(on)), "gyp_ingest_get_level"),
                           (lambda: lib.gyp_ingest_calibrate(h, 0, 2, 1, 1.0, 0.0, None, None), "gyp_ingest_calibrate")):
            assert call() == BAD and (lib.gyp_last_error(None) or b"").decode().startswith(name)
        assert on.value == 7 and out["gain"][0] == 0      # nothing was written
        # the host-only reader itself is untouched
        raw, first, n_ms = C.c_void_p(), C.c_int64(), C.c_int32()
        assert lib.gyp_ingest_next_host(h, C.byref(raw), C.byref(first), C.byref(n_ms)) == 0 and (first.value, n_ms.value) == (0, 1)
        assert lib.gyp_ingest_set_level(None, None) == BAD and lib.gyp_ingest_get_level(None, None, None) == BAD
        assert lib.gyp_ingest_calibrate(None, 0, 2, 1, 1.0, 0.0, None, None) == BAD
    finally:
        lib.gyp_ingest_close(h)
