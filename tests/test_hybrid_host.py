"""Weak-signal acquisition, the parts that need no GPU: gyp_hybrid_shift and gyp_hybrid_stats against the float64 model bit for bit,
the record layouts against the header, the refusals that need no context, the model's two forms against each other, and the gates of
the end-to-end scene (tests/hybrid_scene.py) on the model alone -- what tests/test_gpu_hybrid.py then holds the device to."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import hybrid_model as hm
import hybrid_scene as hs
from gypsum_amd import _lib, engine
from oracle import gypsum_oracle as orc

REPO = Path(__file__).resolve().parents[1]
HEADER = REPO / "include" / "gypsum_hip.h"


@pytest.fixture(scope="module")
def lib():
    from gypsum_amd import build
    build.build(verbose=False)
    return _lib.load()


# ---------------------------------------------------------------------------------------------- gyp_hybrid_shift
def test_shift_matches_the_model_bit_for_bit(lib):
    rng = np.random.default_rng(20261020)
    checked = 0
    for T in (1, 4, 10, 20):
        blocks = sorted({0, 1, 2, 3, 7, 21, 99, 100, 1000, 6552, 6553} | set(int(b) for b in rng.integers(0, 6554, 40)))
        for n in (1023, 2046, 3069, 8184):
            for b in blocks:
                if b * T > 65535:
                    continue
                for f in (0.0, 1.0, 4487.0, 7000.0, 200000.0, float(rng.uniform(0, 10000)), float(rng.uniform(0, 1e6))):
                    for sign in (1.0, -1.0):
                        want = hm.shift(n, T, b, sign * f, hm.CODE_DOPPLER)
                        assert lib.gyp_hybrid_shift(n, T, b, sign * f, _lib.GYP_HYB_CODE_DOPPLER) == want
                        assert lib.gyp_hybrid_shift(n, T, b, sign * f, _lib.GYP_HYB_CODE_DOPPLER | _lib.GYP_HYB_ALTERNATE) == want
                        assert lib.gyp_hybrid_shift(n, T, b, sign * f, 0) == 0
                        assert lib.gyp_hybrid_shift(n, T, b, sign * f, _lib.GYP_HYB_ALTERNATE) == 0
                        checked += 1
    assert checked > 5000
    assert engine.hybrid_shift(2046, 10, 21, 4487.0, 2) == hm.shift(2046, 10, 21, 4487.0, 2) == 1


def test_shift_rounds_exact_halves_away_from_zero(lib):
    """Half-way cases by hand: for an elapsed sample count e = b T N the Doppler f = (2 k + 1) 1575420000 / (2 e) makes the quotient
    k + 1/2 exactly -- where f itself is a float64 (1575420000 = 1540 * 1023000, so f = (2 k + 1) 770000 / (e / 1023): exact for
    e / 1023 = 1, 2, 4, 10, 11, 16, 20, and for 3 or 15 when 2 k + 1 is a multiple of it); then e * f = (2 k + 1) 787710000 is an
    integer below 2^53 and its quotient by 1575420000 is exact too.  Cases whose f is no float64 are left out by the Fraction test."""
    from fractions import Fraction
    cases = []
    for n, T, b in ((1023, 1, 1), (2046, 1, 1), (1023, 4, 1), (1023, 4, 4), (2046, 4, 2), (1023, 10, 1), (3069, 1, 1), (3069, 1, 5),
                    (1023, 20, 1), (1023, 1, 11), (8184, 1, 2), (2046, 10, 1)):
        e = b * T * n
        for k in (0, 1, 2, 7, 100, 3000):
            exact = Fraction((2 * k + 1) * 1575420000, 2 * e)
            f = float(exact)
            if Fraction(f) != exact:
                continue
            q = float(e) * f / 1575420000.0
            assert q == k + 0.5, (n, T, b, k)                     # the case really is an exact half in float64
            cases.append((n, T, b, f, k + 1))
    assert {c[0] for c in cases} == {1023, 2046, 3069, 8184}
    for n, T, b, f, want in cases:
        assert lib.gyp_hybrid_shift(n, T, b, f, 2) == want == hm.shift(n, T, b, f, 2)
        assert lib.gyp_hybrid_shift(n, T, b, -f, 2) == -want == hm.shift(n, T, b, -f, 2)
        below, above = math.nextafter(f, 0.0), math.nextafter(f, math.inf)
        assert lib.gyp_hybrid_shift(n, T, b, below, 2) == hm.shift(n, T, b, below, 2)
        assert lib.gyp_hybrid_shift(n, T, b, above, 2) == hm.shift(n, T, b, above, 2)
    assert len(cases) >= 40


# ---------------------------------------------------------------------------------------------- gyp_hybrid_stats
def _record(peak, second, n_off, sum_off, sumsq_off):
    r = np.zeros(1, dtype=_lib.HYBRID_CELL)
    r["peak"], r["second"], r["n_off"], r["sum_off"], r["sumsq_off"] = peak, second, n_off, sum_off, sumsq_off
    return r


def _lib_stats(lib, rec):
    z, ratio = C.c_double(), C.c_double()
    assert lib.gyp_hybrid_stats(_lib.ptr(rec), C.byref(z), C.byref(ratio)) == 0
    return z.value, ratio.value


def _same(a: float, b: float, rel: float = 1e-15) -> bool:
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= rel * abs(b)


def test_stats_match_the_model(lib):
    rng = np.random.default_rng(7)
    for _ in range(2000):
        n_off = int(rng.integers(1, 50000))
        v = rng.gamma(11.0, float(rng.uniform(1e-6, 1e3)), size=min(n_off, 64))
        mean, var = float(v.mean()), float(v.var()) + 1e-30
        rec = _record(np.float32(mean + rng.uniform(0, 40) * math.sqrt(var)), np.float32(mean + 3 * math.sqrt(var)), n_off,
                      mean * n_off, (var + mean * mean) * n_off)
        got, want = _lib_stats(lib, rec), hm.stats(rec[0])
        assert _same(got[0], want[0]) and _same(got[1], want[1]), (rec, got, want)
    z, ratio = engine.hybrid_stats(rec)
    assert z.shape == (1,) and z[0] == got[0] and ratio[0] == got[1]


def test_stats_edge_cases(lib):
    # no lag away from the peak
    z, ratio = _lib_stats(lib, _record(5.0, 0.0, 0, 0.0, 0.0))
    assert math.isnan(z) and ratio == math.inf
    assert math.isnan(hm.stats(_record(5.0, 0.0, 0, 0.0, 0.0)[0])[0])
    # a constant floor: the variance is 0
    rec = _record(5.0, 2.0, 100, 200.0, 400.0)
    z, ratio = _lib_stats(lib, rec)
    assert math.isnan(z) and ratio == 2.5 and math.isnan(hm.stats(rec[0])[0])
    # a variance that cancellation makes negative
    rec = _record(5.0, 2.0, 3, 0.3, 0.03 * (1 - 1e-15))
    assert math.isnan(_lib_stats(lib, rec)[0]) and math.isnan(hm.stats(rec[0])[0])
    # second = 0 -> inf; 0 / 0 -> NaN
    assert _lib_stats(lib, _record(1.0, 0.0, 10, 1.0, 1.0))[1] == math.inf == hm.stats(_record(1.0, 0.0, 10, 1.0, 1.0)[0])[1]
    assert math.isnan(_lib_stats(lib, _record(0.0, 0.0, 10, 1.0, 1.0))[1])
    # either output may be left out; a NULL record is refused
    z = C.c_double()
    assert lib.gyp_hybrid_stats(_lib.ptr(_record(4.0, 1.0, 4, 4.0, 8.0)), C.byref(z), None) == 0 and z.value == 3.0
    assert lib.gyp_hybrid_stats(_lib.ptr(_record(4.0, 1.0, 4, 4.0, 8.0)), None, None) == 0
    assert lib.gyp_hybrid_stats(None, C.byref(z), None) == _lib.GYP_E_BAD_ARG
    assert b"gyp_hybrid_stats" in lib.gyp_last_error(None)


# ---------------------------------------------------------------------------------------------- layouts, refusals
def test_hybrid_record_layouts_match_the_header(tmp_path):
    structs = {"gyp_hybrid_cell": _lib.HYBRID_CELL, "gyp_weak_result": _lib.WEAK_RESULT}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for name, dt in structs.items():
        lines.append(f'printf("{name} size %zu\\n", sizeof({name}));')
        for field in dt.names:
            lines.append(f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    lines.append('printf("flags x %d\\n", GYP_HYB_ALTERNATE * 10 + GYP_HYB_CODE_DOPPLER);')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out.strip().splitlines()}
    for name, dt in structs.items():
        assert got[(name, "size")] == dt.itemsize == _lib.RECORD_SIZES[name], name
        for field in dt.names:
            assert got[(name, field)] == dt.fields[field][1], (name, field)
    assert _lib.HYBRID_CELL.itemsize == 48 and _lib.WEAK_RESULT.itemsize == 56
    assert got[("flags", "x")] == _lib.GYP_HYB_ALTERNATE * 10 + _lib.GYP_HYB_CODE_DOPPLER == 12
    # field for field into a gyp_chan_init
    for field in ("stream", "sat_id", "doppler_hz", "carrier_phase", "code_phase"):
        assert _lib.WEAK_RESULT.fields[field][0] == _lib.CHAN_INIT.fields[field][0], field


def test_entry_points_refuse_a_missing_context(lib):
    buf = np.zeros(16, dtype=np.float32)
    ids = np.array([1], dtype=np.int32)
    bins = np.array([0.0])
    out = np.zeros(1, dtype=_lib.HYBRID_CELL)
    wout = np.zeros(1, dtype=_lib.WEAK_RESULT)
    p = _lib.ptr
    assert lib.gyp_correlate_grid_hybrid_dev(None, p(buf), 1, 0, 10, 2, 3, p(ids), 1, p(bins), 1, p(out)) == _lib.GYP_E_BAD_ARG
    assert lib.gyp_correlate_grid_hybrid(None, p(buf), 1, 10, 2, 3, p(ids), 1, p(bins), 1, p(out)) == _lib.GYP_E_BAD_ARG
    assert lib.gyp_acquire_weak_dev(None, p(buf), 1, 0, 10, 2, 3, 0.0, 7000.0, 10.0, p(ids), 1, p(wout)) == _lib.GYP_E_BAD_ARG
    assert lib.gyp_acquire_weak(None, p(buf), 1, 10, 2, 3, 0.0, 7000.0, 10.0, p(ids), 1, p(wout)) == _lib.GYP_E_BAD_ARG
    assert not out.tobytes().strip(b"\0") and not wout.tobytes().strip(b"\0")


def test_model_refuses_what_the_library_refuses():
    x = np.zeros(2046 * 2, dtype=np.complex64)
    for T, M, flags in ((0, 1, 0), (21, 1, 0), (10, 0, 0), (10, 6554, 0), (1, 1, hm.ALTERNATE), (1, 2, 4), (1, 2, 8 | 1)):
        with pytest.raises(ValueError):
            hm.hybrid_cell(x, 2_046_000, 2046, 1, 0.0, T, M, flags)


# ---------------------------------------------------------------------------------------------- the model itself
def test_the_models_shared_form_equals_the_oracle_form():
    """block_profiles_shared (what the searches over thousands of cells use) against block_profiles (oracle.integrate_correlation per
    block), and the level's bins."""
    x = hs.iq()
    for sats, f, T, M in (((3, 7), -2870.0, 10, 3), ((19,), 4487.5, 3, 4), ((26, 1, 32), 200000.0, 20, 2), ((5,), 0.0, 1, 5)):
        shared = hm.block_profiles_shared(x, hs.FS, hs.N, sats, f, T, M)
        for k, sv in enumerate(sats):
            want = hm.block_profiles(x, hs.FS, hs.N, sv, f, T, M)
            assert np.abs(shared[k] - want).max() <= 1e-9 * np.abs(want).max()
    bins = hm.coarse_bins(0.0, 7000.0, 10)
    assert len(bins) == 280 and bins[0] == -7000.0 and bins[-1] == 6950.0 and bins[1] - bins[0] == 50.0
    assert hm.coarse_bins(100.0, 500.0, 20) == [-400.0 + 25.0 * i for i in range(40)]
    assert hm.fine_bins(1250.0, 10.0, 10) == [1250.0 + 10.0 * j for j in range(-2, 3)]
    assert hm.fine_bins(0.0, 0.0, 10) == [] and hm.fine_bins(0.0, -1.0, 10) == [] and hm.fine_bins(5.0, 300.0, 1) == [5.0]


def test_rendered_peak_really_drifts():
    """With code Doppler rendered, a strong noiseless satellite's coherent peak moves one sample per 1 / (f / 1575.42e6) samples, to
    where gyp_hybrid_shift says; without it the peak stays."""
    from gypsum_amd import synth
    sat = synth.SyntheticSatellite(sat_id=9, doppler_hz=200000.0, code_phase=1, carrier_phase=0.3, amplitude=1.0)
    sc = synth.SyntheticScene(fs=hs.FS, n_ms=8, sats=[sat], noise_sigma=0.0, seed=1)
    for f in (200000.0, -200000.0):
        sat.doppler_hz = f
        x, still = hm.render(sc, code_doppler=True), hm.render(sc, code_doppler=False)
        np.testing.assert_array_equal(still, synth.render(sc))        # no code Doppler: synth.render itself
        C = hm.block_profiles(x, hs.FS, hs.N, 9, f, 1, 8)
        peaks = [int(np.argmax(np.abs(c))) for c in C]
        want = [(1 - hm.shift(hs.N, 1, b, f, hm.CODE_DOPPLER)) % hs.N for b in range(8)]
        assert len(set(peaks)) >= 3                                   # it moves ...
        # ... to within the half sample by which the drift inside a block and the rounding may differ
        assert all(min((p - w) % hs.N, (w - p) % hs.N) <= 1 for p, w in zip(peaks, want)), (peaks, want)
        assert peaks[0] == 1 and (peaks[7] - 1 + hs.N // 2) % hs.N - hs.N // 2 == -hm.shift(hs.N, 1, 7, f, hm.CODE_DOPPLER)
        assert [int(np.argmax(np.abs(c))) for c in hm.block_profiles(still, hs.FS, hs.N, 9, f, 1, 8)] == [1] * 8


# ---------------------------------------------------------------------------------------------- gates of the end-to-end scene
def drift_corrected_truth(sat) -> int:
    """Where the aligned power profile peaks: the code phase at the buffer's first sample (block 0 carries no shift)."""
    return sat.code_phase % hs.N


def circ(a: int, b: int) -> int:
    d = abs(a - b) % hs.N
    return min(d, hs.N - d)


def test_scene_is_what_the_gates_need():
    tr = hs.truth()
    assert sorted(tr) == sorted(hs.WEAK + hs.STRONG)
    for sv in hs.WEAK:
        assert abs(hs.cn0_of_scene(tr[sv].amplitude, hs.SIGMA, hs.N) - 30.0) < 1e-9
    assert abs(hs.cn0_of_scene(tr[3].amplitude, hs.SIGMA, hs.N) - 45.0) < 1e-9
    d = [s.doppler_hz for s in tr.values()]
    assert min(d) < -4400 and max(d) > 4400 and max(abs(v) for v in d) <= 4500
    cps = [s.code_phase for s in tr.values()]
    assert 0 in cps and hs.N - 1 in cps
    offs = [s.nav_bit_offset_ms for s in tr.values()]
    assert len(set(offs)) == 4 and any(o % 10 == 0 for o in offs) and tr[7].nav_bit_offset_ms % 10 == 5
    assert all(s.nav_bits is not None for s in tr.values())
    assert hs.N_MS == 220 and hs.FS == 2_046_000 and hs.M * hs.T == hs.N_MS


def test_reference_search_misses_the_weak_satellites():
    """oracle.detect_satellites on the first 10 ms: the strong satellite, none of the three weak ones."""
    x10 = hs.iq()[:10 * hs.N]
    tr = hs.truth()
    codes = orc.generate_ca_codes()
    replicas = {sv: orc.prn_as_complex(codes[sv - 1], hs.N) for sv in tr}
    found = {r.satellite_id: r for r in orc.detect_satellites(sorted(tr), x10, hs.FS, hs.N, replicas)}
    assert not set(found) & set(hs.WEAK)
    assert 3 in found and found[3].prn_phase_shift == tr[3].code_phase


def test_model_search_finds_all_four_and_nothing_else():
    from gypsum_amd.acquisition import DEFAULT_WEAK_Z_THRESHOLD
    tr, res = hs.truth(), hs.model_results()
    for sv, sat in tr.items():
        r = res[sv]
        print(f"sat {sv}: z {r.z:.3f} doppler {r.doppler_hz} (true {sat.doppler_hz}) code phase {r.code_phase} (true {sat.code_phase}) margin {r.z_margin:.3g}")
        assert r.z > DEFAULT_WEAK_Z_THRESHOLD
        assert circ(r.code_phase, drift_corrected_truth(sat)) <= 1
        assert abs(r.doppler_hz - sat.doppler_hz) <= hs.FINE_STEP_HZ
        # the device decides the same bins only if float32 cannot reorder them: the seed was chosen with room
        assert r.z_margin > 1e-3
    rest = {sv: res[sv].z for sv in hs.ALL_SATS if sv not in tr}
    print(f"largest z of the 28 absent satellites: {max(rest.values()):.3f} (threshold {DEFAULT_WEAK_Z_THRESHOLD})")
    assert len(rest) == 28 and max(rest.values()) < DEFAULT_WEAK_Z_THRESHOLD


def test_recorded_model_answers_are_the_models():
    """tests/golden/hybrid_scene.npz (what the GPU tests compare the device with) against the model run afresh."""
    fresh, rec = hs.golden_arrays(hs.model_results()), hs.golden_arrays(hs.golden_results())
    for k in hs.GOLDEN_FIELDS:
        if fresh[k].dtype.kind == "f":
            np.testing.assert_allclose(rec[k], fresh[k], rtol=1e-9, atol=1e-12, err_msg=k)
        else:
            np.testing.assert_array_equal(rec[k], fresh[k], err_msg=k)


def test_each_flag_matters_on_the_scene():
    both = {sv: hs.z_at_truth(hs.SEED, sv, hs.FLAGS) for sv in hs.WEAK}
    for sv in (7, 19):                                    # the +-4.5 kHz satellites: 1.3 samples of drift over 220 ms
        no_cd = hs.z_at_truth(hs.SEED, sv, hm.ALTERNATE)
        print(f"sat {sv}: z {both[sv]:.3f} with both flags, {no_cd:.3f} without CODE_DOPPLER")
        assert no_cd < both[sv]
    no_alt = hs.z_at_truth(hs.SEED, 7, hm.CODE_DOPPLER)   # bit edges in the middle of the odd blocks
    print(f"sat 7: z {both[7]:.3f} with both flags, {no_alt:.3f} without ALTERNATE")
    assert no_alt < both[7]
    assert hs.flips_at_edges(hs.truth()[7]) >= 7
    assert hs.model_results()[7].set == 0                 # the even blocks are the clean ones
