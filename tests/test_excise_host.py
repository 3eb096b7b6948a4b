"""The excisor's host side (no GPU): gyp_excise_from_hist against tests/excise_model.py bit for bit, every argument rule, the record
layout, the ingest entry points on a handle without a context, the model's own invariants, and the gates of the two end-to-end
scenes: the oracle misses planted satellites under the jammer, raw and notched, and finds all four once the model has excised it."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import excise_model as model
import notch_model
from gypsum_amd import _lib
from gypsum_amd import excisor as ex
from oracle import gypsum_oracle as orc

HEADER = Path(__file__).resolve().parents[1] / "include" / "gypsum_hip.h"
BAD = _lib.GYP_E_BAD_ARG


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def clean_hist():
    return model.spectrum_hist(model.scene("fm", 2)[1], model.SCENE_N)


# ---------------------------------------------------------------------------------------------------- gyp_excise_from_hist
def _histograms(clean_hist):
    out = {"the clean scene": (clean_hist, 16.0, 1), "another factor and guard": (clean_hist, 9.5, 8)}
    one = np.zeros(model.BINS, dtype=np.uint32)
    one[1017] = 7
    out["one bin"] = (one, 16.0, 0)
    edge = np.zeros(model.BINS, dtype=np.uint32)
    edge[[900, 1016, 1030]] = [5, 15, 20]                  # M = 40, r = 20 = the cumulative count of bin 1016 exactly
    out["the rank on a bin's edge"] = (edge, 4.0, 1)
    odd = np.zeros(model.BINS, dtype=np.uint32)
    odd[[0, 1, 2039]] = [1, 1, 1]                           # r = 1.5 inside bin 1: a denormal median
    out["a denormal median"] = (odd, 16.0, 4)
    tail = clean_hist.copy()
    tail[2040:] = 1000                                      # non-finite powers do not count
    out["non-finite powers are left out"] = (tail, 16.0, 1)
    return out


@pytest.mark.parametrize("name", ["the clean scene", "another factor and guard", "one bin", "the rank on a bin's edge", "a denormal median",
                                  "non-finite powers are left out"])
def test_from_hist_equals_the_model_bit_for_bit(lib, clean_hist, name):
    h, factor, guard = _histograms(clean_hist)[name]
    want, median, t = model.from_hist(h, factor, guard)
    got, measured = ex.excisor_from_hist(h, factor, guard)
    print(f"{name}: median {median!r} threshold {t!r}")
    assert np.float64(measured["median"]).tobytes() == np.float64(median).tobytes()
    assert np.float64(measured["threshold"]).tobytes() == np.float64(t).tobytes()
    assert (got.threshold, got.guard) == tuple(want)
    if name == "the rank on a bin's edge":
        assert median == ex_bin_edges()[1017]
    if name == "one bin":
        e = ex_bin_edges()
        assert median == e[1017] + 0.5 * (e[1018] - e[1017])
    if name == "non-finite powers are left out":
        assert want == model.from_hist(clean_hist)[0]


def ex_bin_edges():
    import blank_model
    return blank_model.bin_edges()


def test_from_hist_shares_the_blankers_arithmetic(lib, clean_hist):
    from gypsum_amd import blanker as bk
    for factor in (16.0, 7.25):
        b, mb = bk.blanker_from_hist(clean_hist, (0.0, 0.0), factor, 4)
        e, me = ex.excisor_from_hist(clean_hist, factor, 4)
        assert mb == me and b.threshold == e.threshold


def test_from_hist_refuses_bad_arguments(lib, clean_hist):
    h = clean_hist
    rec, m = np.zeros(1, dtype=ex.EXCISOR_DTYPE), np.full(2, 7.0)

    def refused(rc, what):
        msg = (lib.gyp_last_error(None) or b"").decode()
        assert rc == BAD and msg.startswith("gyp_excise_from_hist"), (what, rc, msg)

    refused(lib.gyp_excise_from_hist(None, 16.0, 1, _lib.ptr(rec), _lib.ptr(m)), "hist NULL")
    refused(lib.gyp_excise_from_hist(_lib.ptr(h), 16.0, 1, None, _lib.ptr(m)), "excisor_out NULL")
    for v in (0.0, -1.0, np.inf, np.nan):
        refused(lib.gyp_excise_from_hist(_lib.ptr(h), v, 1, _lib.ptr(rec), _lib.ptr(m)), f"factor {v}")
    for g in (-1, 9):
        refused(lib.gyp_excise_from_hist(_lib.ptr(h), 16.0, g, _lib.ptr(rec), _lib.ptr(m)), f"guard {g}")
    empty = np.zeros(model.BINS, dtype=np.uint32)
    refused(lib.gyp_excise_from_hist(_lib.ptr(empty), 16.0, 1, _lib.ptr(rec), _lib.ptr(m)), "M = 0")
    empty[2040:] = 9
    refused(lib.gyp_excise_from_hist(_lib.ptr(empty), 16.0, 1, _lib.ptr(rec), _lib.ptr(m)), "only non-finite powers")
    huge = np.zeros(model.BINS, dtype=np.uint32)
    huge[2039] = 3                                          # its upper edge is +inf: the threshold does not fit float32
    refused(lib.gyp_excise_from_hist(_lib.ptr(huge), 16.0, 1, _lib.ptr(rec), _lib.ptr(m)), "a threshold float32 cannot hold")
    huge[:] = 0
    huge[2030] = 3
    refused(lib.gyp_excise_from_hist(_lib.ptr(huge), 1e45, 1, _lib.ptr(rec), _lib.ptr(m)), "a threshold beyond float32")
    tiny = np.zeros(model.BINS, dtype=np.uint32)
    tiny[0] = 3
    refused(lib.gyp_excise_from_hist(_lib.ptr(tiny), 1e-60, 1, _lib.ptr(rec), _lib.ptr(m)), "a threshold that rounds to 0")
    assert rec["threshold"][0] == 0.0 and (m == 7.0).all()                      # a refused call writes no excisor
    assert lib.gyp_excise_from_hist(_lib.ptr(h), 16.0, 8, _lib.ptr(rec), None) == 0 and rec["guard"][0] == 8
    assert (rec["reserved"] == 0).all()
    with pytest.raises(_lib.GypsumHipError, match="gyp_excise_from_hist"):
        ex.excisor_from_hist(h, 0.0, 1)
    with pytest.raises(ValueError):
        ex.excisor_from_hist(h[:100])


def test_the_python_mirror_of_the_rules(lib):
    ex.check_excisor(ex.Excisor(1.0, 0))
    ex.check_excisor(ex.Excisor(1e-30, 8))
    for bad in (ex.Excisor(0.0, 0), ex.Excisor(-1.0, 0), ex.Excisor(np.inf, 0), ex.Excisor(np.nan, 0), ex.Excisor(1e39, 0), ex.Excisor(1e-46, 0),
                ex.Excisor(1.0, -1), ex.Excisor(1.0, 9), ex.Excisor(1.0, 1.5)):
        with pytest.raises(ValueError):
            ex.check_excisor(bad)
    e = ex.Excisor(4.25, 7)
    assert ex.Excisor.from_record(e.record()) == e
    assert len(ex.excisor_records(e, 3)) == 3 and len(ex.excisor_records([e, e])) == 2
    for n in (1, 100, 128, 129, 255, 256, 257, 2046, 49104, 65536):
        assert ex.n_frames(n) == model.n_frames(n) == -(-(n + 128) // 128)
    assert ex.FRAME == model.FRAME == 256 and ex.MAX_GUARD == model.MAX_GUARD == 8


def test_the_record_layout_matches_the_header(tmp_path):
    dt = _lib.EXCISOR
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("gyp_excisor size %zu\\n", sizeof(gyp_excisor));']
    for field in dt.names:
        lines.append(f'printf("gyp_excisor {field} %zu\\n", offsetof(gyp_excisor, {field}));')
    lines.append('printf("excise frame %d\\n", GYP_EXCISE_FRAME);')
    lines.append('printf("reserved words %zu\\n", sizeof(((gyp_excisor*)0)->reserved) / sizeof(int32_t));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {(l.split()[0], l.split()[1]): int(l.split()[2]) for l in out}
    assert got[("gyp_excisor", "size")] == dt.itemsize == _lib.RECORD_SIZES["gyp_excisor"] == 16
    for field in dt.names:
        assert got[("gyp_excisor", field)] == dt.fields[field][1], field
    assert got[("excise", "frame")] == _lib.GYP_EXCISE_FRAME == 256 and got[("reserved", "words")] == 2


def test_a_handle_without_a_context_has_no_excisor(lib, tmp_path):
    path = tmp_path / "x.bin"
    np.zeros(2 * 2046 * 5, dtype=np.uint8).tofile(path)
    h = C.c_void_p()
    assert lib.gyp_ingest_open(None, str(path).encode(), _lib.GYP_FMT_U8, 2_046_000, 2046, 1, 3, C.byref(h)) == 0
    try:
        rec, on, n = ex.Excisor(3.0, 1).record(), C.c_int32(7), C.c_int32(7)
        out, m, counts = np.zeros(1, dtype=ex.EXCISOR_DTYPE), np.full(2, 7.0), np.full(4, 7, dtype=np.int32)
        for call, name in ((lambda: lib.gyp_ingest_set_excisor(h, _lib.ptr(rec)), "gyp_ingest_set_excisor"),
                           (lambda: lib.gyp_ingest_set_excisor(h, None), "gyp_ingest_set_excisor"),
                           (lambda: lib.gyp_ingest_get_excisor(h, _lib.ptr(out), C.byref(on)), "gyp_ingest_get_excisor"),
                           (lambda: lib.gyp_ingest_find_excisor(h, 0, 2, 16.0, 1, 1, _lib.ptr(out), _lib.ptr(m)), "gyp_ingest_find_excisor"),
                           (lambda: lib.gyp_ingest_last_excised(h, _lib.ptr(counts), 4, C.byref(n)), "gyp_ingest_last_excised")):
            assert call() == BAD and (lib.gyp_last_error(None) or b"").decode().startswith(name), name
        assert on.value == 7 and n.value == 7 and (m == 7.0).all() and (counts == 7).all() and out["threshold"][0] == 0.0
        raw, first, n_ms = C.c_void_p(), C.c_int64(), C.c_int32()
        assert lib.gyp_ingest_next_host(h, C.byref(raw), C.byref(first), C.byref(n_ms)) == 0 and (first.value, n_ms.value) == (0, 1)
        assert lib.gyp_ingest_set_excisor(None, None) == BAD and lib.gyp_ingest_get_excisor(None, None, None) == BAD
        assert lib.gyp_ingest_find_excisor(None, 0, 2, 16.0, 1, 0, None, None) == BAD
        assert lib.gyp_ingest_last_excised(None, None, 0, None) == BAD
    finally:
        lib.gyp_ingest_close(h)


def test_bad_calls_are_refused_before_the_device_is_touched(lib):
    """NULL buffers and a NULL context: the calls return GYP_E_BAD_ARG without a launch; the rules themselves are checked with a
    context in tests/test_gpu_excise.py."""
    one = ex.Excisor(3.0, 1).record()
    assert lib.gyp_excise_iq_dev(None, None, None, 1, 0, 1, 2046, _lib.ptr(one), None, None) == BAD
    assert (lib.gyp_last_error(None) or b"").decode().startswith("gyp_excise_iq_dev")
    assert lib.gyp_iq_spectrum_hist_dev(None, None, 1, 0, 1, 2046, None) == BAD
    assert (lib.gyp_last_error(None) or b"").decode().startswith("gyp_iq_spectrum_hist_dev")


# ---------------------------------------------------------------------------------------------------- the model itself
def test_the_window_halves_sum_to_one_within_one_ulp():
    w = model.window()
    assert w.dtype == np.float32 and w[0] == 0.0 and w[128] == 1.0
    s = w[:128].astype(np.float64) + w[128:].astype(np.float64)
    assert np.abs(s - 1.0).max() <= np.spacing(np.float32(1.0))


def test_every_sample_lies_in_exactly_two_frames():
    for n in (1, 100, 128, 129, 255, 256, 257, 1023, 2046):
        fr = model.frames(np.arange(1, n + 1, dtype=np.float64))
        assert fr.shape == (model.n_frames(n), 256)
        assert np.array_equal(np.bincount(fr[fr > 0].astype(int), minlength=n + 1)[1:], np.full(n, 2))


def test_the_model_with_nothing_hit_returns_the_inputs_bits():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(3 * 300) + 1j * rng.standard_normal(3 * 300)).astype(np.complex64)
    x[7] = np.complex64(complex(-0.0, np.nan))
    x[400] = -0.0
    for f in (model.excise, model.excise32):
        y, masks, counts = f(x, 300, model.Excisor(1e6, 3))
        assert np.array_equal(y.view(np.uint64), x.view(np.uint64)) and not masks.any() and not counts.any()


def test_the_model_excises_a_tone_and_its_circular_guard_and_leaves_other_milliseconds_alone():
    n = 512
    i = np.arange(3 * n)
    rng = np.random.default_rng(6)
    x = 0.01 * (rng.standard_normal(3 * n) + 1j * rng.standard_normal(3 * n))
    x[n:2 * n] += np.exp(-2j * np.pi * 0.5 / 256 * i[n:2 * n])                  # half a bin below 0: bins 255 and 0
    x = x.astype(np.complex64)
    y, masks, counts = model.excise(x, n, model.Excisor(20.0, 2))
    cut = model.unpack_masks(masks)
    assert not cut[0].any() and not cut[2].any() and counts[0] == counts[2] == 0
    assert np.array_equal(y[:n].view(np.uint64), x[:n].view(np.uint64)) and np.array_equal(y[2 * n:].view(np.uint64), x[2 * n:].view(np.uint64))
    inner = cut[1][1:-1]                                                        # the frames inside the millisecond
    assert inner[:, [253, 254, 255, 0, 1, 2]].all() and not inner[:, 8:248].any()   # the guard wraps round the ring
    assert counts[1] == cut[1].sum()
    assert np.abs(y[n + 128:2 * n - 128]).max() < 0.1                           # the tone is gone where both frames are whole
    y2, masks2, _ = model.excise(x, n, model.Excisor(1e-3, 0), masks=masks)     # given decisions are applied, not remade
    assert np.array_equal(masks2, masks) and np.array_equal(y2.view(np.uint64), y.view(np.uint64))
    y32, masks32, _ = model.excise32(x, n, model.Excisor(20.0, 2))
    assert np.array_equal(masks32, masks) and np.abs(y32 - y).max() < 1e-5


def test_masks_pack_bin_k_into_bit_k():
    cut = np.zeros((2, 256), dtype=bool)
    cut[0, [0, 63, 64, 255]] = True
    w = model.pack_masks(cut)
    assert w[0].tolist() == [1 | (1 << 63), 1, 0, 1 << 63] and not w[1].any()
    assert np.array_equal(model.unpack_masks(w), cut)


def test_the_models_histogram_counts_full_frames_only():
    rng = np.random.default_rng(7)
    for n, full in ((256, 1), (383, 1), (384, 2), (2046, 14)):
        x = (rng.standard_normal(2 * n) + 1j * rng.standard_normal(2 * n)).astype(np.complex64)
        assert len(model.full_frames(n)) == full and model.spectrum_hist(x, n).sum() == 256 * full * 2


# ---------------------------------------------------------------------------------------------------- the scenes' gates
@pytest.mark.parametrize("kind", ["fm", "sweep"])
def test_the_jammer_hides_the_satellites_raw_and_notched_and_the_model_excisor_uncovers_all_four(kind):
    """Raw, and notched at the jammer's centre frequency, the oracle's acquisition misses planted satellites (a miss: a wrong code
    phase, a Doppler more than 50 Hz off, or a strength of at most the oracle's threshold of 3); with the model excisor from the
    model's histogram (full frames only, factor 16, guard 1) it finds all four."""
    x, clean = model.scene(kind, 10)
    e, median, t = model.from_hist(model.spectrum_hist(x, model.SCENE_N), 16.0, 1)
    y, masks, counts = model.excise(x, model.SCENE_N, e)
    notched = notch_model.notch(x, model.SCENE_FS, model.SCENE_N, [notch_model.SCENE_TONE_HZ])
    notched = notched[0] if isinstance(notched, tuple) else notched
    chips = orc.generate_ca_codes()

    def found(data, what):
        ok = []
        for sv, (cp, doppler) in model.SCENE_SATS.items():
            o = orc.acquire_satellite(sv, np.asarray(data, dtype=np.complex128), model.SCENE_FS, model.SCENE_N,
                                      orc.prn_as_complex(chips[sv - 1], model.SCENE_N))
            print(f"{kind} {what} PRN {sv}: Doppler {o.doppler_shift} code phase {o.prn_phase_shift} strength {o.correlation_strength:.2f}; "
                  f"planted {doppler} {cp}")
            ok.append(o.prn_phase_shift == cp and abs(o.doppler_shift - doppler) <= 50.0
                      and o.correlation_strength > orc.ACQUISITION_STRENGTH_THRESHOLD)
        return ok

    share = counts.sum() / masks[..., 0].size / 256
    print(f"{kind}: median {median:.5f} threshold {t:.5f} excised share of (frame, bin) cells {share:.4f}")
    assert sum(found(x, "raw")) < 4
    assert sum(found(notched, "notched")) < 4
    assert all(found(y, "excised"))
    assert model.excise(clean, model.SCENE_N, e)[2].sum() <= 2e-4 * masks[..., 0].size * 256   # (one clean bin in 65536 is expected)
