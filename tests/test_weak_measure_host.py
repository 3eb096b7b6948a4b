"""Weak-signal measurement, the parts that need no GPU: the record layouts and the defaults against the header and the model,
gyp_weak_measure_estimate and gyp_weak_measured_state against the float64 model (tests/weak_measure_model.py) -- bit for bit where
only + - x / and sqrt are involved -- every refusal that needs no context, and the gates of the estimator on the model's scene: what
tests/test_gpu_weak_measure.py then holds the device to.

Measured on the model (python tests/weak_measure_model.py): 2.046 Msps, sample-centre rendering with code Doppler, seeds 1..8, the
start the integer sample nearest a code phase drawn uniformly within half a sample, Doppler 0.2 Hz off, two passes, d = 0.5 chip:

    scene                       drift (samples)  start rms  final rms  largest  C/N0 mean  largest C/N0 error
    30 dB-Hz  4487 Hz  220 ms   1.28             0.105      0.043      0.068    29.59      1.04 dB     gated
    33 dB-Hz -3950 Hz  220 ms   1.13             0.158      0.039      0.071    32.72      0.61 dB     gated
    45 dB-Hz  4100 Hz  220 ms   1.17             0.181      0.013      0.023    44.61      0.59 dB     gated
    30 dB-Hz  1233 Hz 1000 ms   1.60             0.128      0.016      0.028    29.84      0.58 dB     gated
    30 dB-Hz  1233 Hz  220 ms   0.35             0.147      0.197      0.348    29.89      1.02 dB     lattice-limited: printed only
    45 dB-Hz -2871 Hz  220 ms   0.82             0.181      0.040      0.084    44.90      0.28 dB     lattice-limited: printed only

(errors of c0 in chips).  The gate on the C/N0 is the model's largest error over the seeds times 1.5 (CN0_MARGIN_DB below).  Where the
code drifts less than one sample across the buffer the early-late difference is a staircase in the code offset with a dead zone: at
0.35 samples of drift the correction does not improve on the sample grid, and may step away from it.
"""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import weak_measure_model as mm
import weak_track_model as wm
from gypsum_amd import _lib, _records, engine

REPO = Path(__file__).resolve().parents[1]
HEADER = REPO / "include" / "gypsum_hip.h"
BAD_ARG = _lib.GYP_E_BAD_ARG
# the model's largest |C/N0 estimate - scene's| over SEEDS (above), times 1.5, per gated scene in mm.SCENES order
CN0_MARGIN_DB = (1.043 * 1.5, 0.605 * 1.5, 0.590 * 1.5, 0.577 * 1.5)


@pytest.fixture(scope="module")
def lib():
    from gypsum_amd import build
    build.build(verbose=False)
    return _lib.load()


# ---------------------------------------------------------------------------------------------- layouts and defaults
def test_measure_record_layouts_match_the_header(tmp_path):
    structs = {"gyp_weak_measure_params": _lib.WEAK_MEASURE_PARAMS, "gyp_weak_measured": _lib.WEAK_MEASURED, "gyp_weak_measure_fold": _lib.WEAK_MEASURE_FOLD}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for name, dt in structs.items():
        lines.append(f'printf("{name} size %zu\\n", sizeof({name}));')
        for field in dt.names:
            lines.append(f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
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
    assert [dt.itemsize for dt in structs.values()] == [16, 80, 64]
    # the offsets the header states
    m = _lib.WEAK_MEASURED.fields
    assert [m[k][1] for k in _lib.WEAK_MEASURED.names] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 76]
    assert _lib.GYP_VERSION == 209


def test_defaults_are_the_models(lib):
    d = engine.weak_measure_params_default()[0]
    m = mm.Params()
    assert (int(d["spacing"]), int(d["passes"]), int(d["reserved"])) == (m.spacing, m.passes, 0) == (1 << 39, 2, 0)
    assert _records.WeakMeasureParams().record().tobytes() == engine.weak_measure_params_default().tobytes()
    assert _records.WeakMeasureParams.from_record(engine.weak_measure_params_default()) == _records.WeakMeasureParams()


# ---------------------------------------------------------------------------------------------- the twin against the model
def records(minus, prompt, plus) -> np.ndarray:
    out = np.zeros(len(prompt), dtype=_lib.WEAK_MS_REC)
    for name, v in (("minus", minus), ("prompt", prompt), ("plus", plus)):
        v = np.asarray(v).astype(np.complex64)
        out[name + "_re"], out[name + "_im"] = v.real, v.imag
    return out


def same_fold(got: np.ndarray, want: mm.Fold) -> None:
    """Bit for bit in everything but the C/N0 (log10)."""
    for name in ("e_minus", "e_prompt", "e_plus", "wn", "dd"):
        assert float(got[name]) == getattr(want, name), (name, float(got[name]), getattr(want, name))
    assert (int(got["c0"]), int(got["n_groups"]), int(got["status"])) == (want.c0, want.n_groups, want.status)
    g = float(got["cn0_dbhz"])
    assert (math.isnan(g) and math.isnan(want.cn0_dbhz)) or abs(g - want.cn0_dbhz) <= 1e-9


def synthetic(n_ms, seed, late=0.2, amp=30.0, noise=1.0, w_mean=2.0):
    """Per-millisecond sums of a replica `late` chips late (a triangle of half-width 1 chip at d = 1/2), with data bits every 20 ms
    from millisecond 0 of the buffer, and W_m about w_mean."""
    rng = np.random.default_rng([seed, n_ms])
    bits = np.repeat(rng.integers(0, 2, n_ms // 20 + 1) * 2 - 1, 20)[:n_ms]
    ph = np.exp(1j * rng.uniform(-np.pi, np.pi))
    lag = lambda o: amp * max(0.0, 1.0 - abs(o - late)) * bits * ph + noise * (rng.standard_normal(n_ms) + 1j * rng.standard_normal(n_ms))
    return lag(-0.5), lag(0.0), lag(0.5), w_mean * (1.0 + 0.1 * rng.standard_normal(n_ms))


def check(minus, prompt, plus, w, first_ms, edge, c0, spacing=1 << 39) -> np.ndarray:
    want = mm.fold(minus, prompt, plus, w, first_ms, edge, spacing, c0)
    got = engine.weak_measure_estimate(records(minus, prompt, plus), w, first_ms, edge, c0, spacing)
    print(f"n_ms {len(w)} first_ms {first_ms} edge {edge} spacing 2^{spacing.bit_length() - 1}: groups {got['n_groups']} dd {got['dd']!r} ({want.dd!r}) "
          f"c0 {got['c0']} ({want.c0}) cn0 {got['cn0_dbhz']!r} ({want.cn0_dbhz!r}) status {got['status']}")
    same_fold(got, want)
    return got


@pytest.mark.parametrize("n_ms, first_ms, edge, spacing", [(40, 0, 0, 1 << 39), (220, 7, 7, 1 << 39), (220, 7, 6, 1 << 38), (2000, 123456, 19, 1 << 36),
                                                           (1000, 19, 0, (1 << 39) - 12345), (47, 1, 0, 1 << 37)])
def test_the_twin_is_the_model_bit_for_bit(lib, n_ms, first_ms, edge, spacing):
    head = (edge - first_ms) % 20
    mi, pr, pl, w = (np.roll(v, head) for v in synthetic(n_ms, n_ms))            # the data bits turn at the group heads
    got = check(mi, pr, pl, w, first_ms, edge, 5 * wm.ONE + 77, spacing)
    assert int(got["n_groups"]) == (n_ms - head) // 20 == mm.n_groups(n_ms, first_ms, edge)


def test_a_late_replica_makes_plus_larger_and_c0_moves_forward(lib):
    mi, pr, pl, w = synthetic(200, 3, late=0.2, noise=0.0, w_mean=1e-3)
    got = check(mi, pr, pl, w, 0, 0, 1000 * wm.ONE)
    # the triangle: A- = 0.3 amp, A+ = 0.7 amp -> dd = 0.5 (0.4 / 1.0) = 0.2 chip, up to the noise share taken off
    assert abs(float(got["dd"]) - 0.2) < 1e-3 and int(got["c0"]) == 1000 * wm.ONE + wm.llround(float(got["dd"]) * wm.ONE)
    early = check(pl, pr, mi, w, 0, 0, 1000 * wm.ONE)
    assert float(early["dd"]) == -float(got["dd"])


def test_a_correction_wraps_c0_through_zero_and_through_the_modulus(lib):
    mi, pr, pl, w = synthetic(100, 4, late=0.25, noise=0.0, w_mean=1e-3)
    up = check(mi, pr, pl, w, 0, 0, wm.CODE_MOD - 1000)                           # forward through 1023 * 2^40
    assert 0 < float(up["dd"]) < 0.5 and int(up["c0"]) == wm.llround(float(up["dd"]) * wm.ONE) - 1000 < wm.ONE
    down = check(pl, pr, mi, w, 0, 0, 1000)                                       # backward through 0
    assert float(down["dd"]) < 0 and int(down["c0"]) == wm.CODE_MOD + 1000 + wm.llround(float(down["dd"]) * wm.ONE) > wm.CODE_MOD - wm.ONE
    check(mi, pr, pl, w, 0, 0, wm.CODE_MOD - 1)
    check(mi, pr, pl, w, 0, 0, 0)


def test_exactly_one_group_with_a_first_ms_that_is_no_multiple_of_twenty(lib):
    first_ms, edge, n_ms = 1013, 5, 40                                            # head = (5 - 13) % 20 = 12: one group at 12..31, 32..39 left over
    mi, pr, pl, w = synthetic(n_ms, 5)
    got = check(mi, pr, pl, w, first_ms, edge, 12345)
    assert int(got["n_groups"]) == 1 and mm.first_head(first_ms, edge) == 12
    # only the group's twenty milliseconds enter: everything outside may change
    for v in (mi, pr, pl, w):
        v[:12] = 99.0
        v[32:] = -99.0
    again = check(mi, pr, pl, w, first_ms, edge, 12345)
    assert again.tobytes() == got.tobytes()
    # and with the head at 0 there are two
    assert int(check(mi, pr, pl, w, first_ms, 13, 12345)["n_groups"]) == 2


def test_all_zero_sums_set_status_bit_1_and_leave_c0(lib):
    z = np.zeros(60, dtype=np.complex64)
    got = check(z, z, z, np.zeros(60), 3, 3, 987654321)
    assert int(got["status"]) == 1 and int(got["c0"]) == 987654321 and float(got["dd"]) == 0.0 and math.isnan(float(got["cn0_dbhz"]))
    assert float(got["wn"]) == 0.0
    got = check(z, z, z, np.full(60, 4.0), 3, 3, 987654321)                       # noise power but no sums
    assert int(got["status"]) == 1 and int(got["c0"]) == 987654321 and math.isnan(float(got["cn0_dbhz"]))


def test_a_noise_only_row_is_clamped(lib):
    rng = np.random.default_rng(6)
    n_ms = 100
    noise = lambda: (rng.standard_normal(n_ms) + 1j * rng.standard_normal(n_ms)).astype(np.complex64)       # E ~ 40 per group
    w = np.full(n_ms, 50.0)                                                        # Wn = 1000 per group: every E is below it
    got = check(noise(), noise(), noise(), w, 0, 0, 4242)
    assert float(got["e_minus"]) < float(got["wn"]) and float(got["e_plus"]) < float(got["wn"]) and float(got["e_prompt"]) < float(got["wn"])
    assert int(got["status"]) == 1 and int(got["c0"]) == 4242 and float(got["dd"]) == 0.0 and math.isnan(float(got["cn0_dbhz"]))
    # one side above the noise share, the other below: the clamp makes dd the full (1 - d), not a NaN
    mi, pl = noise(), noise()
    pl[:20] += 10.0
    got = check(mi, noise(), pl, np.full(n_ms, 2.0), 0, 0, 4242)
    assert float(got["e_minus"]) < float(got["wn"]) < float(got["e_plus"])
    assert int(got["status"]) == 0 and float(got["dd"]) == 0.5 and int(got["c0"]) == 4242 + wm.ONE // 2


def test_refusals(lib):
    s = np.zeros(100, dtype=_lib.WEAK_MS_REC)
    w = np.zeros(100)
    out = np.full(64, 7, dtype=np.uint8)
    p = _lib.ptr

    def est(sums=s, ww=w, n_ms=100, first=0, edge=0, spacing=1 << 39, c0=0, o=out):
        return lib.gyp_weak_measure_estimate(None if sums is None else p(sums), None if ww is None else p(ww), n_ms, first, edge, spacing, c0,
                                             None if o is None else p(o))

    for what, kw in (("NULL sums", dict(sums=None)), ("NULL w", dict(ww=None)), ("NULL out", dict(o=None)), ("spacing below 2^36", dict(spacing=(1 << 36) - 1)),
                     ("spacing above 2^39", dict(spacing=(1 << 39) + 1)), ("spacing 0", dict(spacing=0)), ("n_ms 39", dict(n_ms=39)), ("n_ms 2001", dict(n_ms=2001)),
                     ("first_ms < 0", dict(first=-1)), ("edge -1", dict(edge=-1)), ("edge 20", dict(edge=20)), ("c0 < 0", dict(c0=-1)),
                     ("c0 at the modulus", dict(c0=wm.CODE_MOD))):
        assert est(**kw) == BAD_ARG, what
        assert lib.gyp_last_error(None), what
        want = mm.refusal(mm.Params(spacing=kw.get("spacing", 1 << 39)), kw.get("n_ms", 100), kw.get("first", 0)) or mm.edge_refusal(kw.get("edge", 0), 100, 0)
        if want:
            assert lib.gyp_last_error(None).decode().endswith(want), (what, lib.gyp_last_error(None))
    assert np.all(out == 7)
    assert est(spacing=1 << 36) == 0 and est(n_ms=40) == 0 and est(edge=19, c0=wm.CODE_MOD - 1) == 0
    # the model's refusals of a whole request, in the header's order
    assert mm.refusal(mm.Params(passes=0), 100, 0) == mm.refusal(mm.Params(passes=5), 100, 0) == "passes must be 1..4"
    assert mm.refusal(mm.Params(spacing=1, passes=0), 10, -1) == "spacing must be 2^36 .. 2^39"
    assert mm.cand_refusal(0, 5, 1.0, 0.0, 2046, 0, 2046, 100, 0) == "a code phase is outside [0, N)"
    assert mm.cand_refusal(0, 5, 1.0, 0.0, 2045, 20, 2046, 100, 0) == "an edge is outside 0..19"
    assert all(mm.n_groups(40, f, e) >= 1 for f in range(40) for e in range(20))          # 40 ms always hold a whole group
    # the state
    rec = np.zeros(1, dtype=_lib.WEAK_MEASURED)
    st = np.full(64, 7, dtype=np.uint8)

    def state(r=rec, fs=2_046_000, n=2046, ahead=0, o=st, **kw):
        r = None if r is None else r.copy()
        for k, v in kw.items():
            r[k] = v
        return lib.gyp_weak_measured_state(None if r is None else p(r), fs, n, ahead, None if o is None else p(o))

    for what, kw in (("NULL record", dict(r=None)), ("NULL out", dict(o=None)), ("fs 0", dict(fs=0)), ("N 0", dict(n=0)), ("N 2047", dict(n=2047)),
                     ("ms_ahead -1", dict(ahead=-1)), ("ms_ahead 65536", dict(ahead=65536)), ("NaN Doppler", dict(doppler_hz=np.nan)),
                     ("infinite phase", dict(carrier_phase=np.inf)), ("c0 -1", dict(c0=-1)), ("c0 at the modulus", dict(c0=wm.CODE_MOD)),
                     ("edge -1", dict(edge=-1)), ("edge 20", dict(edge=20))):
        assert state(**kw) == BAD_ARG, what
    assert np.all(st == 7) and state() == 0


@pytest.mark.parametrize("fs, n", [(1_023_000, 1023), (2_046_000, 2046), (49_104_000, 49104)])
def test_the_state_is_the_model_stepped_by_hand(lib, fs, n):
    rec = np.zeros(1, dtype=_lib.WEAK_MEASURED)
    rec["stream"], rec["sat_id"], rec["doppler_hz"], rec["carrier_phase"], rec["c0"], rec["edge"] = 1, 9, -4321.987, -2.5, 1022 * wm.ONE + 999, 17
    for ahead in (0, 1, 40, 220, 2000):
        got = engine.weak_measured_state(rec, fs, n, ahead)
        want = mm.state(-4321.987, -2.5, 1022 * wm.ONE + 999, 17, fs, n, ahead)
        assert (float(got["f"]), float(got["f_int"]), float(got["u0"]), int(got["c0"]), int(got["phase"]), int(got["edge"])) == \
            (want["f"], want["f_int"], want["u0"], want["c0"], wm.WAIT, 17), ahead
        assert (int(got["status"]), int(got["pos"]), int(got["n_periods"]), float(got["mu_mean"])) == (0, 0, 0, 0.0)
    # a carrier phase a hair below zero: u0 is 0, as in the bank's start rule
    rec["carrier_phase"] = -1e-300
    assert float(engine.weak_measured_state(rec, fs, n, 0)["u0"]) == 0.0
    # and the code phase in samples inverts the start rule
    # (exactly where (0.5 - code_phase) / K is a whole number of 2^-40 chips, K = 1 and 2; to c0's resolution, K 2^-41 samples, at K = 48)
    for cp in (0, 1, n // 3, n - 1):
        back = mm.code_phase_samples(wm.init_c0(cp, n), n)
        assert 0.0 <= back < n and abs((back - cp + n / 2) % n - n / 2) <= (0.0 if n <= 2046 else 48 * 2.0 ** -41 + n * 2.0 ** -52)


# ---------------------------------------------------------------------------------------------- the model's scene
_figures = {}


def scene(index: int) -> dict:
    """One scene of mm.SCENES over mm.SEEDS: the model's sums, folded pass by pass through the library's host form (which must agree
    with the model's own fold bit for bit), and the errors against the rendered truth."""
    if index in _figures:
        return _figures[index]
    name, sv, cn0, doppler, n_ms, gated = mm.SCENES[index]
    start, final, cn0_err = [], [], []
    for seed in mm.SEEDS:
        s, x, c = mm.one_case(sv, cn0, doppler, n_ms, seed)
        m = mm.measure(x, mm.chips_pm(sv), mm.FS, mm.N, c["doppler_hz"], c["carrier_phase"], c["code_phase"], c["edge"], c["first_ms"], n_ms, keep=True)
        c0 = wm.init_c0(c["code_phase"], mm.N)
        for (mi, pr, pl), w, fo in zip(m.sums, m.w, m.folds):
            got = engine.weak_measure_estimate(records(mi, pr, pl), w, c["first_ms"], c["edge"], c0)
            same_fold(got, fo)
            c0 = int(got["c0"])
        assert c0 == m.c0 and m.status == 0 and m.n_groups == mm.n_groups(n_ms, c["first_ms"], c["edge"])
        start.append(mm.code_error(wm.init_c0(c["code_phase"], mm.N), s, mm.N))
        final.append(mm.code_error(c0, s, mm.N))
        cn0_err.append(float(got["cn0_dbhz"]) - cn0)
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
    _figures[index] = dict(name=name, gated=gated, start_rms=rms(start), final_rms=rms(final), final_max=float(np.max(np.abs(final))),
                           cn0_mean=cn0 + float(np.mean(cn0_err)), cn0_err_max=float(np.max(np.abs(cn0_err))), drift=mm.drift_samples(doppler, n_ms))
    g = _figures[index]
    print(f"{name} (drift {g['drift']:.2f} samples): start rms {g['start_rms']:.4f} final rms {g['final_rms']:.4f} largest {g['final_max']:.4f} chip; "
          f"C/N0 mean {g['cn0_mean']:.3f}, largest error {g['cn0_err_max']:.3f} dB")
    return g


GATED = [i for i, s in enumerate(mm.SCENES) if s[5]]
LATTICE = [i for i, s in enumerate(mm.SCENES) if not s[5]]


@pytest.mark.parametrize("index", GATED)
def test_where_the_code_drifts_a_sample_the_error_halves_and_the_cn0_is_the_scenes(lib, index):
    g = scene(index)
    assert g["drift"] >= 1.0
    assert abs(g["start_rms"] - 0.5 / math.sqrt(12)) < 0.06                       # the sample grid's: uniform within half a sample = a quarter chip
    assert g["final_rms"] < 0.5 * g["start_rms"]
    assert g["cn0_err_max"] <= CN0_MARGIN_DB[GATED.index(index)]
    assert {mm.SCENES[i][2] for i in GATED} == {30.0, 33.0, 45.0} and len(mm.SEEDS) >= 8


@pytest.mark.parametrize("index", LATTICE)
def test_lattice_limited_scenes_are_printed_not_gated(lib, index):
    g = scene(index)
    assert g["drift"] < 1.0 and math.isfinite(g["final_rms"]) and math.isfinite(g["cn0_mean"])


# ---------------------------------------------------------------------------------------------- the route, on the model alone
def test_the_route_passes_on_the_model_and_the_golden_file_records_it():
    """What tests/test_gpu_weak_measure.py asks of the device on mm.route_iq(), asked of the model first (ROUTE_SEED was chosen so; seeds
    1 and 3 pass as well), from the search results the golden file records (the model's search takes ten seconds: --write-golden)."""
    g = mm.route_golden()
    rows = mm.route_model(search=[(float(f), float(ph), int(cp)) for f, ph, cp in g["search"]])
    for i, r in enumerate(rows):
        s, fig, m = r["sat"], mm.route_figures(r), r["measured"]
        print(f"satellite {s.sat_id}: code error {r['start_error']:+.3f} -> {r['code_error']:+.3f} chip, C/N0 {m.cn0_dbhz:.2f}, {fig}")
        assert int(g["search"][i][2]) == round(s.code_phase) and abs(float(g["search"][i][0]) - s.doppler_hz) <= 10.0
        assert (m.c0, r["edge"], fig["wrong"], fig["n_bits"], fig["first_a"], fig["first_b"]) == \
            (int(g["c0"][i]), int(g["edge"][i]), int(g["wrong"][i]), int(g["n_bits"][i]), int(g["first_measured"][i]), int(g["first_sync"][i]))
        assert r["edge"] == (-s.bit_offset_ms) % 20 and m.status == 0
        assert fig["wrong"] == 0 and fig["n_bits"] == (mm.ROUTE_MS - fig["first_a"]) // 20              # every bit from the first whole period
        assert fig["first_a"] == r["edge"] and fig["first_b"] - fig["first_a"] >= 400
        assert fig["dd_a"] < fig["dd_b"]
        assert abs(r["code_error"]) < abs(r["start_error"]) and abs(m.cn0_dbhz - 30.0) <= CN0_MARGIN_DB[0]
