"""Weak-signal hand-over, the parts that need no GPU: the record layouts and the defaults against the header and the model,
gyp_weak_refine_estimate against the float64 model (tests/weak_refine_model.py) on constructed prompts, every refusal that needs no
context, and the gates of the search -> refine -> bank route on the model alone -- what tests/test_gpu_weak_refine.py then holds the
device to.

Measured on the model (python tests/weak_refine_model.py 99 322), each FAR_BIN_STARTS start of tests/weak_track_scene.py refined on
the scene's first 220 ms from carrier phase 0.3 and the true code phase, then tracked over the scene from the refined start:

    seed  sat  start   refined error  edge (true)  phase error (mod pi)  peak/mean  edge ratio  wrong bits  phase rms
    99    7    -7 Hz   +0.111 Hz      15 (15)      -0.094 rad            48.5       1.06        0 of 89     0.239
    99    19   -8 Hz   -0.054 Hz      10 (10)      +0.077 rad            38.9       1.07        0 of 89     0.174
    99    26   +7 Hz   -0.242 Hz      7 (7)        +0.220 rad            32.0       1.23        0 of 89     0.236
    322   7    -7 Hz   +0.011 Hz      15 (15)      -0.006 rad            36.1       1.07        0 of 89     0.220
    322   19   -8 Hz   -0.177 Hz      10 (10)      +0.013 rad            45.0       1.15        0 of 89     0.289
    322   26   +7 Hz   -0.159 Hz      7 (7)        +0.115 rad            48.8       1.04        0 of 89     0.169

With the code phase one sample (half a chip) off the refined errors are +0.078, -0.258, -0.157, -0.001, +0.348 and -0.082 Hz and
peak/mean falls to 5.7 .. 13.2.
"""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import weak_refine_model as rm
import weak_track_scene as ws
from gypsum_amd import _lib, _records, engine

REPO = Path(__file__).resolve().parents[1]
HEADER = REPO / "include" / "gypsum_hip.h"


@pytest.fixture(scope="module")
def lib():
    from gypsum_amd import build
    build.build(verbose=False)
    return _lib.load()


# ---------------------------------------------------------------------------------------------- layouts and defaults
def test_refine_record_layouts_match_the_header(tmp_path):
    structs = {"gyp_weak_refine_params": _lib.WEAK_REFINE_PARAMS, "gyp_weak_refined": _lib.WEAK_REFINED}
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
    assert [dt.itemsize for dt in structs.values()] == [24, 64]
    assert _lib.GYP_VERSION == 209
    # by field name into a gyp_chan_init, as gyp_weak_result does
    assert set(_lib.CHAN_INIT.names) - {"reserved"} <= set(_lib.WEAK_REFINED.names)
    for name in set(_lib.CHAN_INIT.names) - {"reserved"}:
        assert _lib.CHAN_INIT.fields[name][0] == _lib.WEAK_REFINED.fields[name][0], name


def test_defaults_are_the_models(lib):
    d = engine.weak_refine_params_default()[0]
    m = rm.Params()
    assert (float(d["span_hz"]), float(d["step_hz"]), int(d["presum_ms"]), int(d["reserved"])) == (m.span_hz, m.step_hz, m.presum_ms, 0) == (20.0, 0.5, 4, 0)
    assert _records.WeakRefineParams().record().tobytes() == engine.weak_refine_params_default().tobytes()
    assert _records.WeakRefineParams.from_record(engine.weak_refine_params_default()) == _records.WeakRefineParams()
    assert rm.shape(m, 220) == (4, 55, 40, 10)


# ---------------------------------------------------------------------------------------------- the estimate against the model
def bpsk(n_ms, first_ms, edge, residual_hz, phase, amp=40.0, noise=0.0, seed=1):
    """Prompts of a BPSK signal with a bit edge at every millisecond m with m % 20 == edge, rotating at residual_hz from `phase`."""
    rng = np.random.default_rng([seed, n_ms, first_ms])
    m = first_ms + np.arange(n_ms)
    bits = rng.integers(0, 2, n_ms // 20 + 3) * 2 - 1
    sig = amp * bits[(m - edge) // 20 - (first_ms - edge) // 20] * np.exp(1j * (2 * np.pi * residual_hz * (np.arange(n_ms) + 0.5) / 1000.0 + phase))
    return (sig + noise * (rng.standard_normal(n_ms) + 1j * rng.standard_normal(n_ms))).astype(np.complex64)


def params_record(p: rm.Params):
    return _records.WeakRefineParams(p.span_hz, p.step_hz, p.presum_ms)


def clear_peak(want: rm.Refined) -> bool:
    """The model's P[k] exceeds both neighbours by more than 1e-9 relative: the library's arg-max cannot differ by rounding."""
    k, P = want.bin, want.power
    return all(P[k] > P[j] * (1 + 1e-9) for j in (k - 1, k + 1) if 0 <= j < len(P))


def check(p, first_ms, prm=rm.Params(), tie=False):
    want = rm.estimate(p, first_ms, prm)
    got = engine.weak_refine_estimate(p, first_ms, params_record(prm))
    print(f"n_ms {len(p)} first_ms {first_ms} {prm}: bin {got['bin']} ({want.bin}) delta {got['delta_hz']!r} ({want.delta_hz!r}) phase {got['carrier_phase']!r} "
          f"({want.carrier_phase!r}) edge {got['edge']} ({want.edge}) peak/mean {got['peak_to_mean']!r} ({want.peak_to_mean!r}) "
          f"edge ratio {got['edge_ratio']!r} ({want.edge_ratio!r}) status {got['status']} ({want.status})")
    if not tie:
        assert clear_peak(want)
    assert (int(got["bin"]), int(got["edge"]), int(got["status"])) == (want.bin, want.edge, want.status)
    assert abs(float(got["delta_hz"]) - want.delta_hz) <= 1e-6 and float(got["doppler_hz"]) == float(got["delta_hz"])
    assert abs(float(got["carrier_phase"]) - want.carrier_phase) <= 1e-6
    for name, w in (("peak_to_mean", want.peak_to_mean), ("edge_ratio", want.edge_ratio)):
        g = float(got[name])
        assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-9 * abs(w), name
    assert (int(got["stream"]), int(got["sat_id"]), int(got["code_phase"])) == (0, 0, 0)
    return got, want


def test_estimate_on_a_clean_rotating_bpsk_sequence(lib):
    """No noise, a bit edge at 13 seen from first_ms = 7 (not a multiple of 20), 6.3 Hz of residual Doppler from phase 0.4: the
    parabola through a 220-ms main lobe sampled every 0.5 Hz lands within 0.05 Hz, the phase within 0.03 rad (mod pi)."""
    for residual, phase in ((6.3, 0.4), (-7.8, -1.1), (0.0, 3.0)):
        got, want = check(bpsk(220, 7, 13, residual, phase), 7)
        assert int(got["edge"]) == 13 and int(got["status"]) == 0
        assert abs(float(got["delta_hz"]) - residual) < 0.05
        assert abs((float(got["carrier_phase"]) - phase + math.pi / 2) % math.pi - math.pi / 2) < 0.03
        assert float(got["peak_to_mean"]) > 20.0 and float(got["edge_ratio"]) > 1.05


def test_estimate_under_noise(lib):
    """Prompt SNR 0 dB per millisecond, as at 30 dB-Hz."""
    for seed, residual in ((3, 6.3), (4, -7.8), (5, 2.1)):
        got, want = check(bpsk(220, 7, 13, residual, 0.4, amp=1.0, noise=1.0 / math.sqrt(2), seed=seed), 7)
        assert abs(float(got["delta_hz"]) - residual) < 1.0 and int(got["status"]) == 0


def test_estimate_with_a_tail_shorter_than_the_presum(lib):
    """n_ms no multiple of presum_ms: the tail is dropped from the periodogram, not from the bit-edge energies."""
    p = bpsk(223, 40, 5, -3.4, 1.0, noise=5.0)
    got, want = check(p, 40)
    head = rm.estimate(p[:220], 40)
    assert want.delta_hz == head.delta_hz and want.bin == head.bin and rm.shape(rm.Params(), 223)[1] == 55
    for prm in (rm.Params(20.0, 0.5, 5), rm.Params(10.0, 0.25, 10), rm.Params(12.0, 1.0, 20), rm.Params(20.0, 0.5, 1), rm.Params(20.0, 0.5, 2)):
        check(bpsk(223, 40, 5, -3.4, 1.0, noise=5.0), 40, prm)


def test_estimate_at_the_minimum_of_eight_groups(lib):
    prm = rm.Params(20.0, 0.5, 5)
    assert rm.shape(prm, 40)[:2] == (5, 8)
    got, want = check(bpsk(40, 3, 11, 4.0, 0.2), 3, prm)
    assert abs(float(got["delta_hz"]) - 4.0) < 0.5
    assert not np.any(want.energies == 0.0)                  # 40 ms: every offset has a group


def test_a_residual_beyond_the_span_ends_in_the_end_bin(lib):
    prm = rm.Params(5.0, 0.5, 4)
    for residual, end in ((6.0, 20), (-6.0, 0)):          # the main lobe (nulls 2.3 Hz from the peak) still rises at the end bin
        got, want = check(bpsk(220, 0, 0, residual, 0.0), 0, prm)
        assert int(got["bin"]) == end and int(got["status"]) == 1
        assert float(got["delta_hz"]) == (end - 10) * 0.5       # d = 0: the bin itself


def test_two_equal_largest_bins_give_the_lowest(lib):
    """Prompts that are real or purely imaginary give real s_g, and for real s_g the sums of bins -j and +j are complex conjugates
    term by term (cos is even and sin odd exactly, on both sides): P is mirror-symmetric bit for bit.  With s_g = cos(2 pi 2 (3 Hz) t_g)
    the two largest bins are -3 Hz and +3 Hz, exactly equal; the lower one is reported."""
    L, G, J = 4, 55, 40
    c = np.cos(2 * np.pi * 2 * 3.0 * rm.group_times(L, G))
    p = np.zeros(G * L, dtype=np.complex64)
    p[::L] = np.where(c >= 0, np.sqrt(np.abs(c)), 1j * np.sqrt(np.abs(c)))
    want = rm.estimate(p, 0)
    assert np.array_equal(want.power, want.power[::-1])                     # on the model alone
    assert want.power[J - 6] == want.power[J + 6] == want.power.max() and np.count_nonzero(want.power == want.power.max()) == 2
    assert all(want.power[J - 6] > want.power[j] * (1 + 1e-9) for j in (J - 7, J - 5))
    assert want.bin == J - 6 and want.status == 0 and abs(want.delta_hz + 3.0) < 0.05
    check(p, 0, tie=True)


def test_all_zero_prompts(lib):
    p = np.zeros(220, dtype=np.complex64)
    got, want = check(p, 7, tie=True)
    assert float(got["delta_hz"]) == 0.0 and math.isnan(float(got["peak_to_mean"])) and math.isnan(float(got["edge_ratio"]))
    assert int(got["bin"]) == 40 and int(got["status"]) == 1 and int(got["edge"]) == 0 and float(got["carrier_phase"]) == 0.0


# ---------------------------------------------------------------------------------------------- refusals
def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


REFUSALS = [
    (dict(span_hz=0.0), 220, 0), (dict(span_hz=-1.0), 220, 0), (dict(span_hz=up(100.0), presum_ms=1), 220, 0), (dict(span_hz=float("nan")), 220, 0),
    (dict(step_hz=down(0.01)), 220, 0), (dict(step_hz=up(20.0)), 220, 0), (dict(step_hz=float("nan")), 220, 0), (dict(step_hz=0.0), 220, 0),
    (dict(presum_ms=0), 220, 0), (dict(presum_ms=3), 220, 0), (dict(presum_ms=8), 220, 0), (dict(presum_ms=40), 2000, 0), (dict(presum_ms=-4), 220, 0),
    (dict(span_hz=62.5), 220, 0), (dict(span_hz=12.5, presum_ms=20), 220, 0), (dict(span_hz=100.0, presum_ms=4), 220, 0),
    (dict(span_hz=20.5, step_hz=0.01), 220, 0), (dict(span_hz=100.0, step_hz=0.04, presum_ms=1), 220, 0),
    ({}, 39, 0), ({}, 2001, 0), ({}, 0, 0), ({}, -5, 0),
    (dict(presum_ms=10, span_hz=10.0), 79, 0), (dict(presum_ms=20, span_hz=10.0), 159, 0), (dict(presum_ms=5), 39, 0),
    ({}, 220, -1), ({}, 220, -2 ** 40),
]
ACCEPTED = [
    (dict(span_hz=0.01, step_hz=0.01), 220, 0),
    (dict(span_hz=100.0, step_hz=0.05, presum_ms=2), 220, 0), (dict(span_hz=100.0, step_hz=100.0, presum_ms=1), 220, 0),
    (dict(span_hz=down(62.5)), 220, 0), (dict(span_hz=20.48, step_hz=0.01), 220, 0),
    ({}, 40, 0), ({}, 2000, 0), (dict(presum_ms=10, span_hz=10.0), 80, 0), (dict(presum_ms=20, span_hz=10.0), 160, 2 ** 40), (dict(presum_ms=5), 40, 19),
]


def _request(change):
    rec = engine.weak_refine_params_default()
    for k, v in change.items():
        rec[k] = v
    r = rec[0]
    return rec, rm.Params(float(r["span_hz"]), float(r["step_hz"]), int(r["presum_ms"]))


def test_every_refusal_of_the_estimate(lib):
    """Every refusal of the parameter list that needs no context (the others: tests/test_gpu_weak_refine.py), each beside the nearest
    request that is taken; the model names the same reason.  A refused call leaves *out untouched."""
    p = np.ones(2001, dtype=np.complex64)
    seen = set()
    for change, n_ms, first_ms in REFUSALS:
        rec, prm = _request(change)
        why = rm.refusal(prm, n_ms, first_ms)
        assert why is not None, (change, n_ms, first_ms)
        seen.add(why)
        out = np.full(1, 7, dtype=np.uint8).repeat(64).view(_lib.WEAK_REFINED)
        assert lib.gyp_weak_refine_estimate(_lib.ptr(p), n_ms, first_ms, _lib.ptr(rec), _lib.ptr(out)) == _lib.GYP_E_BAD_ARG, (change, n_ms, first_ms)
        assert out.tobytes() == bytes([7]) * 64
        assert lib.gyp_last_error(None).decode() == "gyp_weak_refine_estimate: " + why
    assert seen == {"span_hz must be in (0, 100]", "step_hz must be in [0.01, span_hz]", "presum_ms must be one of 1, 2, 4, 5, 10, 20",
                    "span_hz must be below 250 / presum_ms", "more than 4097 bins", "n_ms must be 40..2000",
                    "fewer than 8 groups of presum_ms milliseconds", "first_ms is negative"}
    for change, n_ms, first_ms in ACCEPTED:
        rec, prm = _request(change)
        assert rm.refusal(prm, n_ms, first_ms) is None, (change, n_ms, first_ms)
        out = np.zeros(1, dtype=_lib.WEAK_REFINED)
        assert lib.gyp_weak_refine_estimate(_lib.ptr(p), n_ms, first_ms, _lib.ptr(rec), _lib.ptr(out)) == 0, (change, n_ms, first_ms)
    out = np.zeros(1, dtype=_lib.WEAK_REFINED)
    assert lib.gyp_weak_refine_estimate(None, 220, 0, None, _lib.ptr(out)) == _lib.GYP_E_BAD_ARG
    assert lib.gyp_weak_refine_estimate(_lib.ptr(p), 220, 0, None, None) == _lib.GYP_E_BAD_ARG
    assert lib.gyp_weak_refine_estimate(_lib.ptr(p), 220, 0, None, _lib.ptr(out)) == 0          # NULL params: the defaults
    lib.gyp_weak_refine_params_default(None)


def test_entry_points_refuse_a_missing_context(lib):
    p = _lib.ptr
    buf = np.zeros(16, dtype=np.float32)
    res = np.zeros(1, dtype=_lib.WEAK_RESULT)
    out = np.zeros(1, dtype=_lib.WEAK_REFINED)
    assert lib.gyp_weak_refine_dev(None, p(buf), 1, 2046 * 40, 0, 40, p(res), 1, None, p(out), None) == _lib.GYP_E_BAD_ARG
    assert lib.gyp_weak_refine(None, p(buf), 1, 0, 40, p(res), 1, None, p(out), None) == _lib.GYP_E_BAD_ARG
    assert not out.tobytes().strip(b"\0")


# ---------------------------------------------------------------------------------------------- the route, on the model alone
@pytest.fixture(scope="module", params=[99, 322])
def scene_rows(request):
    return rm.scene_rows(request.param)


def test_refined_start_is_within_a_hertz_and_tracks_every_bit(scene_rows):
    """Each start from the search's farther fine bin (7 or 8 Hz off, where the bank false-locks: test_weak_track_host.py), refined on the
    scene's first 220 ms.  The bar of 1 Hz is four times the worst error measured while the estimator was specified and far inside the
    5-Hz pull-in of the bank's loop."""
    assert [r["sat"] for r in scene_rows] == [sv for sv, _ in ws.FAR_BIN_STARTS]
    for r in scene_rows:
        print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
        assert abs(r["start"]) >= 7.0
        assert abs(r["error"]) <= 1.0, r
        assert r["edge"] == r["true_edge"] and r["status"] == 0, r
        assert r["wrong_bits"] == 0 and r["n_bits"] >= 85 and r["phase_rms"] < 0.5 and r["tracked_edge"] == r["true_edge"], r
