"""gyp_weak_refine at its shape edges (the rows of tests/weak_shapes_scene.py; tests/test_weak_shapes_host.py holds the rows to their
conditions first): n_ms % 4 = 1, 2, 3 -- the ragged last workgroup of weak_refine_sums_kernel; 223 ms with presums 4, 5 and 20 -- a
presum tail that the periodogram drops and the bit-edge energies keep, and a finite peak_to_mean; 257 ms at presum 1 -- the second
trip of weak_refine_estimate_kernel's 256-thread loops over n_ms and G; 2000 ms at presum 1 -- G = 2000, every LDS row full; 2000 ms
with 4097 bins; and a residual beyond the span -- status 1 in an end bin.  At each: the prompts bit for bit against a weak bank in SYNC
and against the float64 model's sums, the record against the host twin on the device's own prompts and (within its reach) against the
model, the edge and the Doppler against the scene.

Measured on an MI355X (printed by the tests): the prompts within 2.9e-7 ||x_ms||_2 of the model's sums at every row (bar 1e-4).  The
largest device - twin difference of a row's four candidates, as delta_hz, carrier_phase, peak_to_mean and edge_ratio (relative) -- the
bars are 1e-6 Hz, 1e-6 rad, 1e-9 and 1e-9, and the twin - model difference at these rows is 0 (tests/test_weak_shapes_host.py):

    41, 42, 43 ms, defaults            1.1e-14 Hz  1.3e-15 rad  0             0
    223 ms, presum 4                   0           0            1.5e-16       0
    223 ms, presum 5                   8.9e-16 Hz  6.7e-16 rad  1.5e-16       0
    223 ms, presum 20                  0           0            1.3e-16       0
    257 ms, presum 1                   0           0            3.7e-16       0
    2000 ms, step 0.5, presum 1        0           2.2e-16 rad  2.7e-16       0
    2000 ms, 4097 bins, presum 2       0           0            3.9e-16       0
    223 ms, span 5 (the end bin)       0           0            1.4e-16       0

G = 2000 and 4097 bins stay nine orders inside the bars: the device's sine and cosine differ from the host's in the last bit of a few
terms, and the sums, the parabola and the ratios carry that through unamplified.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import weak_refine_model as rm
import weak_shapes_scene as sc
import weak_track_model as wm
from gypsum_amd import _records

pytestmark = pytest.mark.gpu

ROWS = list(range(len(sc.REFINE_ROWS)))
_cases = {}


def case(engine_factory, k: int) -> dict:
    """Row k refined once through the host form; shared by the tests below and left unchanged."""
    if k in _cases:
        return _cases[k]
    n_ms, p, _, _, _, residuals = sc.REFINE_ROWS[k]
    eng = engine_factory(sc.FS, sc.N)
    x = sc.head_of(sc.refine_iq(), n_ms)
    x.setflags(write=False)
    results = sc.refine_results(residuals)
    rec, prompts = eng.refine_weak(x, 2, sc.FIRST_MS, results, sc.params_record(p), want_prompts=True)
    for a in (rec, prompts):
        a.setflags(write=False)
    _cases[k] = dict(eng=eng, x=x, results=results, rec=rec, prompts=prompts)
    return _cases[k]


@pytest.mark.parametrize("k", ROWS, ids=sc.REFINE_IDS)
def test_prompts_are_a_weak_banks_sync_prompts_and_the_models_sums(engine_factory, k):
    n_ms, p, _, _, _, residuals = sc.REFINE_ROWS[k]
    c = case(engine_factory, k)
    bank = c["eng"].create_weak_bank(sc.inits_of(c["results"]), _records.WeakParams(sync_ms=n_ms), sc.FIRST_MS)
    try:
        ms, _ = bank.track_block(c["x"], 2, sc.FIRST_MS, n_ms, want_periods=False)
    finally:
        bank.close()
    assert np.all(ms["phase"] == wm.SYNC) and np.all(ms["status"] == 0)
    want = np.stack([ms["prompt_re"], ms["prompt_im"]], axis=-1)
    assert want.dtype == np.float32 and c["prompts"].shape == (4, n_ms)
    assert c["prompts"].view(np.float32).reshape(4, n_ms, 2).tobytes() == want.tobytes()
    assert np.count_nonzero(c["prompts"]) == 4 * n_ms
    # the model's sums at the first, the last and three interior milliseconds: the project's 1e-4 ||x_ms||_2 bar
    model = sc.model_sums(residuals, n_ms)
    worst = 0.0
    for i, r in enumerate(c["results"]):
        for m in (0, n_ms // 4, n_ms // 2, (3 * n_ms) // 4, n_ms - 1):
            norm = float(np.linalg.norm(c["x"][int(r["stream"]), m * sc.N:(m + 1) * sc.N].astype(np.complex128)))
            err = abs(complex(c["prompts"][i, m]) - complex(model[i, m]))
            worst = max(worst, err / norm)
            assert err <= 1e-4 * norm, (i, m, err, norm)
    print(f"{sc.REFINE_IDS[k]}: largest |device - model| / ||x_ms||_2 = {worst:.3g}")


@pytest.mark.parametrize("k", ROWS, ids=sc.REFINE_IDS)
def test_records_are_the_twins_the_models_and_the_scenes(engine_factory, k):
    row = sc.REFINE_ROWS[k]
    n_ms, p, G, J, guard, residuals = row
    c = case(engine_factory, k)
    worst = [0.0] * 4
    for i, (r, got) in enumerate(zip(c["results"], c["rec"])):
        f0, phase0 = float(r["doppler_hz"]), float(r["carrier_phase"])
        twin = sc.twin(c["prompts"][i], sc.FIRST_MS, p)
        worst = [max(a, b) for a, b in zip(worst, sc.differences(got, twin, f0, phase0))]
        print(f"{sc.REFINE_IDS[k]} candidate {i}: bin {int(got['bin'])} delta {float(got['delta_hz']):+.6f} (put in {residuals[i]:+.2f}) edge {int(got['edge'])} "
              f"status {int(got['status'])} peak/mean {float(got['peak_to_mean']):.2f} edge ratio {float(got['edge_ratio']):.4f}; "
              f"device - twin {['%.3g' % d for d in sc.differences(got, twin, f0, phase0)]}")
        sc.close_to(got, twin, f0, phase0)
        if sc.within_model(row):            # (beyond it rm.estimate's Python loop over n_bins G terms takes minutes: the 4097-bin row has the twin alone)
            sc.close_to(got, rm.estimate(c["prompts"][i], sc.FIRST_MS, p), f0, phase0)
        assert (int(got["stream"]), int(got["sat_id"]), int(got["code_phase"])) == (int(r["stream"]), int(r["sat_id"]), int(r["code_phase"]))
        assert int(got["edge"]) == sc.refine_true_edge(i)
        if sc.is_end_row(row):
            assert int(got["status"]) == 1 and int(got["bin"]) == (2 * J if residuals[i] > 0 else 0)
            assert float(got["delta_hz"]) == (int(got["bin"]) - J) * p.step_hz and math.isfinite(float(got["peak_to_mean"]))
            continue
        assert int(got["status"]) == 0
        assert math.isnan(float(got["peak_to_mean"])) == (max(int(got["bin"]), 2 * J - int(got["bin"])) <= guard)
        # the main lobe of the squared prompts' periodogram has its nulls 1000 / (2 n_ms) Hz from the peak
        assert abs(float(got["doppler_hz"]) - sc.REFINE_SATS[i][2]) < 500.0 / n_ms
    print(f"{sc.REFINE_IDS[k]}: largest device - twin: delta {worst[0]:.3g} Hz, phase {worst[1]:.3g} rad, peak/mean {worst[2]:.3g}, edge ratio {worst[3]:.3g}")
    if n_ms == 223 and p == sc.DEFAULTS:
        assert all(math.isfinite(float(v)) for v in c["rec"]["peak_to_mean"])          # guard 9: the far-bin mean is computed
