"""Signal quality, host side (no GPU): the record layouts against the header, gyp_quality_from_sums against tests/quality_model.py
on every branch, the model itself on seeded synthetic peaks of known C/N0, and QualityMonitor's bookkeeping against a fake engine
that answers with the model."""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

import quality_model as model
from gypsum_amd import _lib
from gypsum_amd import quality as ql

HEADER = Path(__file__).resolve().parents[1] / "include" / "gypsum_hip.h"
BAD = _lib.GYP_E_BAD_ARG


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_record_layouts_match_the_header(tmp_path):
    structs = {"gyp_quality_sums": _lib.QUALITY_SUMS, "gyp_quality": _lib.QUALITY}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for name, dt in structs.items():
        lines.append(f'printf("{name} size %zu\\n", sizeof({name}));')
        for field in dt.names:
            lines.append(f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    lines.append('printf("gyp_track_rec peak_re %zu\\n", offsetof(gyp_track_rec, peak_re));')
    lines.append('printf("gyp_track_rec locked %zu\\n", offsetof(gyp_track_rec, locked));')
    lines.append('printf("gyp_track_rec status %zu\\n", offsetof(gyp_track_rec, status));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {(l.split()[0], l.split()[1]): int(l.split()[2]) for l in out}
    assert got[("gyp_quality_sums", "size")] == _lib.QUALITY_SUMS.itemsize == _lib.RECORD_SIZES["gyp_quality_sums"] == ql.SUMS_DTYPE.itemsize == 48
    assert got[("gyp_quality", "size")] == _lib.QUALITY.itemsize == _lib.RECORD_SIZES["gyp_quality"] == ql.QUALITY_DTYPE.itemsize == 40
    for name, dt in structs.items():
        for field in dt.names:
            assert got[(name, field)] == dt.fields[field][1], (name, field)
    # what track_quality_kernel reads of a record: the peak at 0, the flag bytes at 49 / 50 of 56
    assert (got[("gyp_track_rec", "peak_re")], got[("gyp_track_rec", "locked")], got[("gyp_track_rec", "status")]) == (0, 49, 50)
    assert _lib.TRACK_REC.itemsize == 56


# ---------------------------------------------------------------------------------------------------- gyp_quality_from_sums
def _sums(n_used=0, n_locked=0, n_groups=0, s2=0.0, s4=0.0, snp=0.0, spl=0.0):
    r = np.zeros(1, dtype=_lib.QUALITY_SUMS)
    r[0] = (n_used, n_locked, n_groups, 0, s2, s4, snp, spl)
    return r


def _call(lib, sums):
    s = np.ascontiguousarray(sums, dtype=_lib.QUALITY_SUMS).reshape(-1)
    out = np.zeros(1, dtype=_lib.QUALITY)
    assert lib.gyp_quality_from_sums(_lib.ptr(s), len(s), _lib.ptr(out)) == 0
    return out[0]


def _same(got, want):
    """Counts and the ratios bit-equal (NaN where the model has NaN); the dB figures within 1e-9 dB (log10 may differ by an ulp)."""
    assert got["n_used"] == want["n_used"] and got["n_groups"] == want["n_groups"]
    for f in ("locked_share", "phase_lock"):
        assert np.array([got[f]]).tobytes() == np.array([want[f]]).tobytes() or (np.isnan(got[f]) and np.isnan(want[f])), f
    for f in ("cn0_m2m4_dbhz", "cn0_nwpr_dbhz"):
        assert np.isnan(got[f]) == np.isnan(want[f]), f
        if not np.isnan(want[f]):
            assert abs(got[f] - want[f]) <= 1e-9, (f, got[f], want[f])


CASES = {
    "both estimators defined": _sums(1000, 700, 50, 1000 * 401.0, 1000 * 162000.0, 50 * 17.5, 50 * 0.93),
    "n_used 1: no moments": _sums(1, 1, 0, 4.0, 16.0),
    "n_used 0: no share either": _sums(0, 0, 0),
    "d < 0 (M4 > 2 M2^2)": _sums(2, 0, 0, 2.0, 5.0),
    "d == 0": _sums(2, 0, 0, 2.0, 4.0),
    "Pn < 0 (sqrt(d) > M2)": _sums(2, 2, 0, 2.0, 1.0),
    "Pn == 0 (M4 == M2^2: no noise)": _sums(4, 0, 0, 4.0, 4.0),
    "no groups": _sums(500, 100, 0, 500 * 3.0, 500 * 17.0),
    "mu below 1": _sums(40, 0, 2, 80.0, 300.0, 1.0, 0.1),
    "mu == 1": _sums(40, 0, 2, 80.0, 300.0, 2.0, 0.1),
    "mu == 20": _sums(40, 0, 2, 80.0, 300.0, 40.0, 2.0),
    "mu above 20": _sums(40, 0, 2, 80.0, 300.0, 41.0, 2.0),
    "mu just inside": _sums(40, 0, 2, 80.0, 300.0, np.nextafter(40.0, 0.0), -1.5),
}


@pytest.mark.parametrize("name", list(CASES))
def test_from_sums_equals_the_model_on_every_branch(lib, name):
    s = CASES[name]
    got, want = _call(lib, s), model.from_sums(s)
    _same(got, want)
    nan = {f for f in ("cn0_m2m4_dbhz", "cn0_nwpr_dbhz", "phase_lock", "locked_share") if np.isnan(got[f])}
    expected_nan = {
        "both estimators defined": set(), "n_used 1: no moments": {"cn0_m2m4_dbhz", "cn0_nwpr_dbhz", "phase_lock"},
        "n_used 0: no share either": {"cn0_m2m4_dbhz", "cn0_nwpr_dbhz", "phase_lock", "locked_share"},
        "d < 0 (M4 > 2 M2^2)": {"cn0_m2m4_dbhz", "cn0_nwpr_dbhz", "phase_lock"}, "d == 0": {"cn0_m2m4_dbhz", "cn0_nwpr_dbhz", "phase_lock"},
        "Pn < 0 (sqrt(d) > M2)": {"cn0_m2m4_dbhz", "cn0_nwpr_dbhz", "phase_lock"},
        "Pn == 0 (M4 == M2^2: no noise)": {"cn0_m2m4_dbhz", "cn0_nwpr_dbhz", "phase_lock"},
        "no groups": {"cn0_nwpr_dbhz", "phase_lock"}, "mu below 1": {"cn0_nwpr_dbhz"}, "mu == 1": {"cn0_nwpr_dbhz"},
        "mu == 20": {"cn0_nwpr_dbhz"}, "mu above 20": {"cn0_nwpr_dbhz"}, "mu just inside": set()}[name]
    assert nan == expected_nan, (name, nan)


def test_from_sums_combines_records_left_to_right(lib):
    rng = np.random.default_rng(11)
    recs = model.records_from_peaks(model.synthetic_peaks(20.0, 1.0, 1000, 13, 5), locked=rng.integers(0, 2, 1000))
    sums = model.track_quality(recs[None, :], 90, [13])[0]           # 12 windows, the last one short
    assert len(sums) == 12
    _same(_call(lib, sums), model.from_sums(sums))
    _same(_call(lib, sums[3:4]), model.from_sums(sums[3:4]))
    q = _call(lib, sums)
    assert q["n_used"] == 1000 and q["locked_share"] == recs["locked"].sum() / 1000.0
    # the binding: per record, and combined along the last axis
    each = ql.from_sums(sums)
    assert each.shape == (12,) and each[3].tobytes() == _call(lib, sums[3:4]).tobytes()
    one = ql.from_sums(sums[3])                                       # a single record gives a single record
    assert one.shape == () and one.tobytes() == each[3].tobytes() and float(one["cn0_m2m4_dbhz"]) == each[3]["cn0_m2m4_dbhz"]
    assert ql.from_sums(sums, combine=True).tobytes() == q.tobytes()
    assert ql.from_sums(np.stack([sums, sums]), combine=True).shape == (2,)


def test_from_sums_bad_arguments(lib):
    s, out = _sums(2, 0, 0, 2.0, 3.0), np.zeros(1, dtype=_lib.QUALITY)
    assert lib.gyp_quality_from_sums(None, 1, _lib.ptr(out)) == BAD
    assert lib.gyp_quality_from_sums(_lib.ptr(s), 1, None) == BAD
    assert lib.gyp_quality_from_sums(_lib.ptr(s), 0, _lib.ptr(out)) == BAD
    assert b"gyp_quality_from_sums" in lib.gyp_last_error(None)
    # the device entry points refuse without a context before anything else
    assert lib.gyp_track_quality_dev(None, None, 1, 1, 1, 1, None, None) == BAD
    assert lib.gyp_track_quality(None, None, 1, 1, 1, 1, None, None) == BAD


def test_cn0_of_scene():
    assert ql.cn0_of_scene(0.01, 0.05, 2046) == pytest.approx(10 * np.log10(1000 * 1e-4 * 2046 / (2 * 25e-4)), abs=1e-12)


# ---------------------------------------------------------------------------------------------------- the model on known C/N0
@pytest.mark.parametrize("a,v", [(20.0, 1.0), (10.0, 5.1)])
def test_model_estimators_on_synthetic_peaks(a, v):
    """A sanity cap, not a measurement: over 20 windows of such input the model's own spread was 0.15-0.25 dB around the truth."""
    truth = 10 * np.log10(1000 * a * a / (2 * v))
    recs = model.records_from_peaks(model.synthetic_peaks(a, v, 1000, 13, seed=3))
    q = model.from_sums(model.track_quality(recs[None, :], 1000, [13])[0])
    print(f"A {a} v {v}: truth {truth:.3f} m2m4 {q['cn0_m2m4_dbhz']:.3f} nwpr {q['cn0_nwpr_dbhz']:.3f} phase_lock {q['phase_lock']:.4f}")
    assert q["n_used"] == 1000 and q["n_groups"] == 49          # groups 13 + 20 g: the one at 993 runs past the window
    assert abs(q["cn0_m2m4_dbhz"] - truth) < 1.0
    assert abs(q["cn0_nwpr_dbhz"] - truth) < 1.0
    assert q["phase_lock"] > 0.9


def test_model_phase_lock_of_noise_is_near_zero():
    recs = model.records_from_peaks(model.synthetic_peaks(0.0, 1.0, 20000, 13, seed=4))
    sums = model.track_quality(recs[None, :], 1000, [13])[0]
    pl = np.array([model.from_sums(s)["phase_lock"] for s in sums])
    print("phase_lock of noise, mean over 20 windows:", pl.mean())
    assert len(pl) == 20 and abs(pl.mean()) < 0.2


# ---------------------------------------------------------------------------------------------------- QualityMonitor
class FakeEngine:
    """Answers track_quality with the model and counts the calls."""

    def __init__(self):
        self.calls = 0

    def track_quality(self, records, window_ms, bit_offsets=None):
        self.calls += 1
        return model.track_quality(records, window_ms, bit_offsets)


N_MON, W_MON, RESET_AT = 1000, 200, 430
BIT_START = [13, 7, None]          # stream index of a record that starts a bit, per channel


@pytest.fixture(scope="module")
def monitor_records():
    recs = np.stack([model.records_from_peaks(model.synthetic_peaks(20.0, 1.0, N_MON, b if b is not None else 0, seed=20 + c))
                     for c, b in enumerate(BIT_START)])
    recs["status"][2, 700:] = 2          # channel 2 is lost from record 700 on
    recs.setflags(write=False)
    return recs


def _run_monitor(recs, block):
    eng = FakeEngine()
    mon = ql.QualityMonitor(eng, 3, W_MON)
    entries = []
    for lo, hi in ((0, RESET_AT), (RESET_AT, N_MON)):       # channel 1 is reset at record RESET_AT
        if lo:
            mon.reset(1)
        for p in range(lo, hi, block):
            e = min(p + block, hi)
            before = eng.calls
            offs = [None if b is None else (b - p) % 20 for b in BIT_START]
            new = mon.push(recs[:, p:e], offs)
            assert eng.calls - before == (1 if new else 0)          # ONE call for all complete windows, none without one
            assert len(mon.last_sums) == len(new)
            entries += [(c, first, q.tobytes(), s.tobytes()) for (c, first, q), s in zip(new, mon.last_sums)]
    return sorted(entries)


def test_monitor_windows_do_not_depend_on_the_blocks(lib, monitor_records):
    recs = monitor_records
    by_block = {b: _run_monitor(recs, b) for b in (250, 97, 1)}
    assert by_block[250] == by_block[97] == by_block[1]
    got = by_block[250]
    # windows count from the channel's reset: channel 1 restarts at RESET_AT and loses the 30 records of its open window
    want = []
    for c, starts in ((0, [(0, w) for w in range(0, 1000, 200)]), (1, [(0, 0), (0, 200), (RESET_AT, 0), (RESET_AT, 200)]),
                      (2, [(0, w) for w in range(0, 1000, 200)])):
        for base, first in starts:
            lo = base + first
            b = -1 if BIT_START[c] is None else (BIT_START[c] - lo) % 20
            s = model.window_sums(recs[c, lo:lo + W_MON], 0, W_MON, b)
            want.append((c, first, model.from_sums(s), s))
    assert sorted((c, f) for c, f, _, _ in got) == sorted((c, f) for c, f, _, _ in want)
    for c, first, q, s in want:
        match = [g for g in got if g[0] == c and g[1] == first and g[3] == s.tobytes()]
        assert len(match) == 1, (c, first)
        _same(np.frombuffer(match[0][2], dtype=_lib.QUALITY)[0], q)
    lost = [np.frombuffer(g[3], dtype=_lib.QUALITY_SUMS)[0] for g in got if g[0] == 2]
    assert [int(s["n_used"]) for s in lost] == [200, 200, 200, 100, 0] and all(s["n_groups"] == 0 for s in lost)


def test_monitor_rejects_bad_shapes():
    with pytest.raises(ValueError):
        ql.QualityMonitor(FakeEngine(), 0, 10)
    mon = ql.QualityMonitor(FakeEngine(), 2, 10)
    with pytest.raises(ValueError):
        mon.push(np.zeros((3, 5), dtype=_lib.TRACK_REC))
    assert mon.push(np.zeros((2, 9), dtype=_lib.TRACK_REC)) == [] and mon.seen(0) == 9
