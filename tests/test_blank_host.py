"""The blanker's host side (no GPU): gyp_blank_from_hist against tests/blank_model.py bit for bit, every argument rule, the record
layout, the ingest entry points on a handle without a context, the model's median against numpy's, and the gate of the end-to-end
scene: the oracle misses the planted satellites under the pulses and finds all four once the model has blanked them."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import blank_model as model
from gypsum_amd import _lib
from gypsum_amd import blanker as bk
from oracle import gypsum_oracle as orc

HEADER = Path(__file__).resolve().parents[1] / "include" / "gypsum_hip.h"
BAD = _lib.GYP_E_BAD_ARG


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def scene10():
    return model.scene(10)


# ---------------------------------------------------------------------------------------------------- gyp_blank_from_hist
def _histograms(scene10):
    x, clean = scene10
    out = {"the scene": (model.hist(x), 0j, 16.0, 4), "its clean twin": (model.hist(clean), 0j, 16.0, 4)}
    out["the scene about a centre"] = (model.hist(x + np.complex64(127.4 + 127.4j), 127.4 + 127.4j), 127.4 + 127.4j, 9.5, 64)
    one = np.zeros(model.BINS, dtype=np.uint32)
    one[1017] = 7
    out["one bin"] = (one, 0j, 16.0, 0)
    edge = np.zeros(model.BINS, dtype=np.uint32)
    edge[[900, 1016, 1030]] = [5, 15, 20]                  # M = 40, r = 20 = the cumulative count of bin 1016 exactly
    out["the rank on a bin's edge"] = (edge, 0j, 4.0, 1)
    odd = np.zeros(model.BINS, dtype=np.uint32)
    odd[[0, 1, 2039]] = [1, 1, 1]                           # r = 1.5 inside bin 1: a denormal median
    out["a denormal median"] = (odd, 0j, 16.0, 4)
    tail = model.hist(clean).copy()
    tail[2040:] = 1000                                      # non-finite powers do not count
    out["non-finite powers are left out"] = (tail, 0j, 16.0, 4)
    return out


@pytest.mark.parametrize("name", ["the scene", "its clean twin", "the scene about a centre", "one bin", "the rank on a bin's edge",
                                  "a denormal median", "non-finite powers are left out"])
def test_from_hist_equals_the_model_bit_for_bit(lib, scene10, name):
    h, c, factor, guard = _histograms(scene10)[name]
    want, median, t = model.from_hist(h, c, factor, guard)
    got, measured = bk.blanker_from_hist(h, (c.real, c.imag), factor, guard)
    print(f"{name}: median {median!r} threshold {t!r}")
    assert np.float64(measured["median"]).tobytes() == np.float64(median).tobytes()
    assert np.float64(measured["threshold"]).tobytes() == np.float64(t).tobytes()
    assert (got.center_re, got.center_im, got.threshold, got.guard) == tuple(want)
    if name == "the rank on a bin's edge":
        assert median == model.bin_edges()[1017]
    if name == "one bin":
        e = model.bin_edges()
        assert median == e[1017] + 0.5 * (e[1018] - e[1017])
    if name == "non-finite powers are left out":
        assert want == model.from_hist(_histograms(scene10)["its clean twin"][0])[0]


def test_from_hist_refuses_bad_arguments(lib, scene10):
    h = model.hist(scene10[1])
    rec, m = np.zeros(1, dtype=bk.BLANKER_DTYPE), np.full(2, 7.0)
    f = C.c_float

    def refused(rc, what):
        msg = (lib.gyp_last_error(None) or b"").decode()
        assert rc == BAD and msg.startswith("gyp_blank_from_hist"), (what, rc, msg)

    refused(lib.gyp_blank_from_hist(None, f(0), f(0), 16.0, 4, _lib.ptr(rec), _lib.ptr(m)), "hist NULL")
    refused(lib.gyp_blank_from_hist(_lib.ptr(h), f(0), f(0), 16.0, 4, None, _lib.ptr(m)), "blanker_out NULL")
    for v in (0.0, -1.0, np.inf, np.nan):
        refused(lib.gyp_blank_from_hist(_lib.ptr(h), f(0), f(0), v, 4, _lib.ptr(rec), _lib.ptr(m)), f"factor {v}")
    for v in (np.inf, -np.inf, np.nan):
        refused(lib.gyp_blank_from_hist(_lib.ptr(h), f(v), f(0), 16.0, 4, _lib.ptr(rec), _lib.ptr(m)), f"center_re {v}")
        refused(lib.gyp_blank_from_hist(_lib.ptr(h), f(0), f(v), 16.0, 4, _lib.ptr(rec), _lib.ptr(m)), f"center_im {v}")
    for g in (-1, 65):
        refused(lib.gyp_blank_from_hist(_lib.ptr(h), f(0), f(0), 16.0, g, _lib.ptr(rec), _lib.ptr(m)), f"guard {g}")
    empty = np.zeros(model.BINS, dtype=np.uint32)
    refused(lib.gyp_blank_from_hist(_lib.ptr(empty), f(0), f(0), 16.0, 4, _lib.ptr(rec), _lib.ptr(m)), "M = 0")
    empty[2040:] = 9
    refused(lib.gyp_blank_from_hist(_lib.ptr(empty), f(0), f(0), 16.0, 4, _lib.ptr(rec), _lib.ptr(m)), "only non-finite powers")
    huge = np.zeros(model.BINS, dtype=np.uint32)
    huge[2039] = 3                                          # its upper edge is +inf: the threshold does not fit float32
    refused(lib.gyp_blank_from_hist(_lib.ptr(huge), f(0), f(0), 16.0, 4, _lib.ptr(rec), _lib.ptr(m)), "a threshold float32 cannot hold")
    huge[:] = 0
    huge[2030] = 3
    refused(lib.gyp_blank_from_hist(_lib.ptr(huge), f(0), f(0), 1e45, 4, _lib.ptr(rec), _lib.ptr(m)), "a threshold beyond float32")
    tiny = np.zeros(model.BINS, dtype=np.uint32)
    tiny[0] = 3
    refused(lib.gyp_blank_from_hist(_lib.ptr(tiny), f(0), f(0), 1e-60, 4, _lib.ptr(rec), _lib.ptr(m)), "a threshold that rounds to 0")
    assert rec["threshold"][0] == 0.0 and (m == 7.0).all()                      # a refused call writes no blanker
    assert lib.gyp_blank_from_hist(_lib.ptr(h), f(0), f(0), 16.0, 4, _lib.ptr(rec), None) == 0 and rec["guard"][0] == 4
    with pytest.raises(_lib.GypsumHipError, match="gyp_blank_from_hist"):
        bk.blanker_from_hist(h, (0.0, 0.0), 0.0, 4)
    with pytest.raises(ValueError):
        bk.blanker_from_hist(h[:100])


def test_the_python_mirror_of_the_rules(lib):
    bk.check_blanker(bk.Blanker(0.0, 0.0, 1.0, 0))
    bk.check_blanker(bk.Blanker(127.4, 127.4, 1e-30, 64))
    for bad in (bk.Blanker(np.inf, 0.0, 1.0, 0), bk.Blanker(0.0, np.nan, 1.0, 0), bk.Blanker(0.0, 0.0, 0.0, 0), bk.Blanker(0.0, 0.0, -1.0, 0),
                bk.Blanker(0.0, 0.0, np.inf, 0), bk.Blanker(0.0, 0.0, 1e39, 0), bk.Blanker(0.0, 0.0, 1e-46, 0), bk.Blanker(0.0, 0.0, 1.0, -1),
                bk.Blanker(0.0, 0.0, 1.0, 65), bk.Blanker(0.0, 0.0, 1.0, 1.5)):
        with pytest.raises(ValueError):
            bk.check_blanker(bad)
    b = bk.Blanker(127.4, -3.0, 4.25, 7)
    assert bk.Blanker.from_record(b.record()) == bk.Blanker(float(np.float32(127.4)), -3.0, 4.25, 7)
    assert len(bk.blanker_records(b, 3)) == 3 and len(bk.blanker_records([b, b])) == 2
    assert np.array_equal(bk.bin_edges()[:2041], model.bin_edges()[:2041]) and bk.bin_edges()[2040] == np.inf and bk.bin_edges()[0] == 0.0
    e = bk.bin_edges()
    assert e[1016] == 1.0 and e[1024] == 2.0 and e[1017] == 1.125                # eighth-octave bins: 3 mantissa bits


def test_the_record_layout_matches_the_header(tmp_path):
    dt = _lib.BLANKER
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("gyp_blanker size %zu\\n", sizeof(gyp_blanker));']
    for field in dt.names:
        lines.append(f'printf("gyp_blanker {field} %zu\\n", offsetof(gyp_blanker, {field}));')
    lines.append('printf("hist bins %d\\n", GYP_POWER_HIST_BINS);')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {(l.split()[0], l.split()[1]): int(l.split()[2]) for l in out}
    assert got[("gyp_blanker", "size")] == dt.itemsize == _lib.RECORD_SIZES["gyp_blanker"] == 16
    for field in dt.names:
        assert got[("gyp_blanker", field)] == dt.fields[field][1], field
    assert got[("hist", "bins")] == _lib.GYP_POWER_HIST_BINS == bk.HIST_BINS == model.BINS == 2048


def test_a_handle_without_a_context_has_no_blanker(lib, tmp_path):
    path = tmp_path / "x.bin"
    np.zeros(2 * 2046 * 5, dtype=np.uint8).tofile(path)
    h = C.c_void_p()
    assert lib.gyp_ingest_open(None, str(path).encode(), _lib.GYP_FMT_U8, 2_046_000, 2046, 1, 3, C.byref(h)) == 0
    try:
        rec, on, n = bk.Blanker(0.0, 0.0, 3.0, 4).record(), C.c_int32(7), C.c_int32(7)
        out, m, counts = np.zeros(1, dtype=bk.BLANKER_DTYPE), np.full(2, 7.0), np.full(4, 7, dtype=np.int32)
        for call, name in ((lambda: lib.gyp_ingest_set_blanker(h, _lib.ptr(rec)), "gyp_ingest_set_blanker"),
                           (lambda: lib.gyp_ingest_set_blanker(h, None), "gyp_ingest_set_blanker"),
                           (lambda: lib.gyp_ingest_get_blanker(h, _lib.ptr(out), C.byref(on)), "gyp_ingest_get_blanker"),
                           (lambda: lib.gyp_ingest_find_pulses(h, 0, 2, 1, 16.0, 4, 1, _lib.ptr(out), _lib.ptr(m)), "gyp_ingest_find_pulses"),
                           (lambda: lib.gyp_ingest_last_blanked(h, _lib.ptr(counts), 4, C.byref(n)), "gyp_ingest_last_blanked")):
            assert call() == BAD and (lib.gyp_last_error(None) or b"").decode().startswith(name), name
        assert on.value == 7 and n.value == 7 and (m == 7.0).all() and (counts == 7).all() and out["threshold"][0] == 0.0
        raw, first, n_ms = C.c_void_p(), C.c_int64(), C.c_int32()
        assert lib.gyp_ingest_next_host(h, C.byref(raw), C.byref(first), C.byref(n_ms)) == 0 and (first.value, n_ms.value) == (0, 1)
        assert lib.gyp_ingest_set_blanker(None, None) == BAD and lib.gyp_ingest_get_blanker(None, None, None) == BAD
        assert lib.gyp_ingest_find_pulses(None, 0, 2, 1, 16.0, 4, 0, None, None) == BAD
        assert lib.gyp_ingest_last_blanked(None, None, 0, None) == BAD
    finally:
        lib.gyp_ingest_close(h)


def test_bad_blankers_are_refused_before_the_device_is_touched(lib):
    """NULL buffers and a NULL context: the calls return GYP_E_BAD_ARG without a launch; the rules themselves are checked with a
    context in tests/test_gpu_blank.py."""
    one = bk.Blanker(0.0, 0.0, 3.0, 4).record()
    assert lib.gyp_blank_iq_dev(None, None, None, 1, 0, 1, 2046, _lib.ptr(one), None) == BAD
    assert (lib.gyp_last_error(None) or b"").decode().startswith("gyp_blank_iq_dev")
    assert lib.gyp_iq_power_hist_dev(None, None, 1, 0, 2046, None, None) == BAD
    assert (lib.gyp_last_error(None) or b"").decode().startswith("gyp_iq_power_hist_dev")


# ---------------------------------------------------------------------------------------------------- the model itself
def test_the_models_median_is_numpys_within_one_percent(scene10):
    """An eighth-octave bin is 9 % wide; the linear interpolation inside it brings the estimate to 0.1 % here."""
    for name, x in zip(("pulsed", "clean"), scene10):
        _, median, _ = model.from_hist(model.hist(x))
        ref = float(np.median(model.power(x).astype(np.float64)))
        print(f"{name}: histogram median {median:.6f}, numpy {ref:.6f}, off by {100 * (median / ref - 1):+.3f} %")
        assert abs(median / ref - 1.0) <= 0.01


def test_the_model_blanks_hits_and_guards_inside_one_millisecond_only():
    n = 200
    x = np.full(3 * n, 0.5 + 0.5j, dtype=np.complex64)
    x[[0, 70, n - 1, 2 * n + 10]] = 10.0
    x[2 * n + 13] = np.nan
    b = model.Blanker(0.0, 0.0, 3.0, 2)
    y, counts = model.blank(x, n, b)
    gone = np.flatnonzero(y.view(np.uint64) != x.view(np.uint64))
    assert gone.tolist() == [0, 1, 2, 68, 69, 70, 71, 72, n - 3, n - 2, n - 1, 2 * n + 8, 2 * n + 9, 2 * n + 10, 2 * n + 11, 2 * n + 12]
    assert counts.tolist() == [11, 0, 5] and (y[gone] == 0).all() and np.isnan(y[2 * n + 13].real)
    y, counts = model.blank(x, n, b._replace(guard=3))
    assert counts.tolist() == [15, 0, 7] and y[2 * n + 13] == 0                 # the NaN is no hit, but a neighbour's guard takes it
    assert y[n] == x[n]                                                         # the hit at n - 1 does not reach into the next millisecond


# ---------------------------------------------------------------------------------------------------- the scene's gate
def test_the_scene_hides_the_satellites_under_the_pulses_and_the_model_blanker_uncovers_all_four(scene10):
    """Un-blanked the oracle's acquisition misses at least three of the four planted satellites (a miss: a wrong code phase, or a
    strength of at most 3); with the model blanker from the model histogram (factor 16, guard 4) it finds all four at the planted
    code phase with a strength above 3; the same blanker blanks no sample of the clean twin; the blanked share lies in [0.10, 0.14].
    Measured: all four missed un-blanked (strengths 1.7 .. 2.0), found at 6.2 .. 6.8 once blanked, 11.96 % blanked."""
    x, clean = scene10
    b, median, t = model.from_hist(model.hist(x), 0j, 16.0, 4)
    y, counts = model.blank(x, model.SCENE_N, b)
    chips = orc.generate_ca_codes()

    def found(data, what):
        ok = []
        for sv, (cp, doppler) in model.SCENE_SATS.items():
            o = orc.acquire_satellite(sv, np.asarray(data, dtype=np.complex128), model.SCENE_FS, model.SCENE_N,
                                      orc.prn_as_complex(chips[sv - 1], model.SCENE_N))
            print(f"{what} PRN {sv}: Doppler {o.doppler_shift} code phase {o.prn_phase_shift} strength {o.correlation_strength:.2f}; planted {doppler} {cp}")
            ok.append(o.prn_phase_shift == cp and o.correlation_strength > 3.0)
        return ok

    share = counts.sum() / len(x)
    print(f"median {median:.5f} threshold {t:.5f} blanked share {share:.4f}")
    assert sum(found(x, "un-blanked")) <= 1
    assert all(found(y, "blanked"))
    assert model.blank(clean, model.SCENE_N, b)[1].sum() == 0
    assert 0.10 <= share <= 0.14
