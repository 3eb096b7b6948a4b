"""The conditions that keep tests/test_gpu_weak_shapes_*.py honest, on the models and the host twins alone (no GPU): every parameter
row of tests/weak_shapes_scene.py is a request that is taken and has the shape its table names; on the model's prompts no row has a
near-tie that the device's sine and cosine could decide the other way; the host twin agrees with the model at these rows inside the
bar the device is then held to against the twin; the end-bin row ends in an end bin.

Measured here (printed by test_twin_agrees_with_the_model_and_nothing_is_near_a_tie): at every row within the model's reach -- all
but the 4097-bin one -- the twin's delta_hz, carrier_phase, peak_to_mean and edge_ratio are the model's, difference 0 on all four
candidates (glibc's sine and cosine gave numpy's bits on these arguments); the bars are 1e-6, 1e-6, 1e-9 and 1e-9.  The smallest
margins: the peak bin over its larger neighbour 1.0001 (41 ms, where the main lobe is 25 Hz wide) and 1.0068 at 4097 bins, 1.04 to
98 elsewhere; the largest bit-edge energy over the second 1.18 to 1.26.
"""
import numpy as np
import pytest

import weak_measure_model as mm
import weak_refine_model as rm
import weak_shapes_scene as sc
import weak_track_model as wm
from gypsum_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from gypsum_amd import build
    build.build(verbose=False)
    return _lib.load()


# ---------------------------------------------------------------------------------------------- requests
def test_refine_rows_are_taken_and_have_the_shapes_named():
    for n_ms, p, G, J, guard, _ in sc.REFINE_ROWS:
        for first_ms in (sc.FIRST_MS, 13, sc.BIG_FIRST_MS):
            assert rm.refusal(p, n_ms, first_ms) is None, (n_ms, p)
        assert rm.shape(p, n_ms) == (p.presum_ms, G, J, guard), (n_ms, p)
    by_id = dict(zip(sc.REFINE_IDS, sc.REFINE_ROWS))
    assert len(by_id) == len(sc.REFINE_ROWS)
    assert [by_id[f"{n}ms-span20-step0.5-presum4"][0] % 4 for n in (41, 42, 43)] == [1, 2, 3]       # the ragged last workgroups
    assert [n_ms % p.presum_ms for n_ms, p, *_ in sc.REFINE_ROWS] == [1, 2, 3, 3, 3, 3, 0, 0, 0, 3]  # the presum tails
    n_ms, p, G, J, _, _ = by_id["2000ms-span64-step0.03125-presum2"]
    assert rm.shape(p, n_ms)[2] == 2048 and 2 * J + 1 == rm.MAX_BINS and n_ms == rm.MAX_MS            # J = 2048 exactly
    assert by_id["2000ms-span20-step0.5-presum1"][2] == rm.MAX_MS                                      # G = 2000
    assert by_id["257ms-span20-step0.5-presum1"][2] > 256                                              # a second trip of 256 threads
    assert [sc.within_model(r) for r in sc.REFINE_ROWS] == [True] * 8 + [False, True]
    assert [sc.is_end_row(r) for r in sc.REFINE_ROWS] == [False] * 9 + [True]
    assert sc.BIG_FIRST_MS % 20 == 9 and (sc.BIG_FIRST_MS & 0xFFFFFFFF) % 20 == 13


def test_measure_rows_are_taken_and_have_the_groups_named():
    for n_ms, start, head, groups in sc.MEASURE_ROWS:
        edge = sc.measure_edge(head)
        assert start + n_ms <= sc.MEASURE_SCENE_MS and (-start) % 20 == head                           # the scene's bits change at 0, 20, ...
        for passes, spacing in sc.SETTINGS:
            assert mm.refusal(mm.Params(spacing, passes), n_ms, sc.FIRST_MS) is None
        assert mm.edge_refusal(edge, n_ms, sc.FIRST_MS) is None
        assert (mm.first_head(sc.FIRST_MS, edge), mm.n_groups(n_ms, sc.FIRST_MS, edge)) == (head, groups), (n_ms, start)
    spare = {(n_ms, head): n_ms - head - 20 * groups for n_ms, _, head, groups in sc.MEASURE_ROWS}
    assert spare[(59, 19)] == 0 and spare[(60, 1)] == 19 and spare[(2000, 0)] == 0 and spare[(2000, 19)] == 1
    assert any(passes == 4 for passes, _ in sc.SETTINGS)
    # the candidate-count and first_ms calls: every edge 0..19 has a whole group in 41 and 43 ms
    for first_ms, n_ms in ((sc.FIRST_MS, 41), (13, 43), (sc.BIG_FIRST_MS, 43)):
        assert all(mm.edge_refusal(e, n_ms, first_ms) is None for e in range(20))
    assert sorted(set(int(e) for e in sc.many_refined(65)["edge"])) == list(range(20))
    for count in (65, 130):
        res = sc.many_results(count)
        assert len(set(zip(res["sat_id"].tolist(), res["doppler_hz"].tolist()))) == count and set(res["stream"].tolist()) == {0, 1}
        assert (count + 63) // 64 >= 2                                                                  # a second workgroup of the plan kernels


def test_bank_rows_are_taken():
    for sync_ms in sc.SYNC_MS:
        assert wm.params_refusal(20, sync_ms, wm.ONE // 2, 8.0, 1.0, 2.5) is None
    assert [s % 20 for s in sc.SYNC_MS] == [0, 7, 1, 0] and max(sc.SYNC_MS) == 2000
    assert sum(sc.SPLIT_47) == 47 + sc.BANK_AFTER_MS and max(sc.SYNC_MS) + sc.BANK_AFTER_MS <= sc.REFINE_SCENE_MS
    assert [(n >> 3, n & 7) for n in sc.BANK_SIZES] == [(1, 0), (1, 1), (1, 5), (2, 1)]
    inits = sc.bank_inits(17)
    assert len(set(zip(inits["sat_id"].tolist(), inits["doppler_hz"].tolist()))) == 17 and set(inits["stream"].tolist()) == {0, 1}
    phase, pos, start = sc.expected_phases(7, 47, 3, 92)
    assert start == 56 and list(phase[45:58]) == [wm.SYNC] * 2 + [wm.WAIT] * 9 + [wm.TRACK] * 2 and list(pos[55:59]) == [0, 0, 1, 2] and pos[76] == 0
    assert sc.expected_phases(0, 40, 0, 85)[2] == 40                                                    # no millisecond of WAIT


# ---------------------------------------------------------------------------------------------- the hand-over's rows on the model
@pytest.mark.parametrize("row", sc.REFINE_ROWS, ids=sc.REFINE_IDS)
def test_twin_agrees_with_the_model_and_nothing_is_near_a_tie(lib, row):
    """On the model's prompts.  The twin against the model is the same class of difference as the device against the twin: the
    platform's sine and cosine.  Where rm.estimate is too slow (n_bins G > 10^6) the no-tie conditions are asked of the twin's own
    output, the peak's margin from three bins of rm.sum_at."""
    n_ms, p, G, J, guard, residuals = row
    prompts = sc.model_prompts(residuals, n_ms)
    worst = [0.0] * 4
    for i in range(4):
        rec = sc.twin_record(prompts[i], sc.FIRST_MS, p)
        got = sc.as_refined(rec)
        if sc.within_model(row):
            want = rm.estimate(prompts[i], sc.FIRST_MS, p)
            sc.close_to(rec, want, 0.0, 0.0)
            worst = [max(a, b) for a, b in zip(worst, sc.differences(rec, want, 0.0, 0.0))]
            k, P = want.bin, want.power
            margin = min(P[k] / P[j] for j in (k - 1, k + 1) if 0 <= j < len(P))
            order = np.sort(want.energies)
            edge_margin = float(order[-1] / order[-2])
            assert want.edge_ratio == edge_margin
        else:
            k, margin, edge_margin = got.bin, sc.peak_margin(prompts[i], p, got.bin), got.edge_ratio
        print(f"{n_ms} ms {p} candidate {i}: bin {got.bin} delta {got.delta_hz:+.6f} (put in {residuals[i]:+.2f}) edge {got.edge} status {got.status} "
              f"peak/mean {got.peak_to_mean:.2f} peak margin {margin:.4f} edge ratio {edge_margin:.4f}")
        assert got.edge == sc.refine_true_edge(i)
        assert margin >= 1 + 1e-9 and edge_margin >= 1 + 1e-6                 # neither bin nor edge can flip on a rounding
        if sc.is_end_row(row):
            assert got.status == 1 and got.bin == (2 * J if residuals[i] > 0 else 0) and got.delta_hz == (got.bin - J) * p.step_hz
            continue
        assert got.status == 0 and 0 < k < 2 * J
        assert abs(got.delta_hz - residuals[i]) < 500.0 / n_ms                # inside the main lobe: nulls 1000 / (2 n_ms) Hz from the peak
        assert np.isnan(got.peak_to_mean) == (max(k, 2 * J - k) <= guard)
    if sc.within_model(row):
        print(f"{n_ms} ms {p}: largest twin - model: delta {worst[0]:.3g} Hz, phase {worst[1]:.3g} rad, peak/mean {worst[2]:.3g}, edge ratio {worst[3]:.3g}")
    if n_ms == 223 and p == sc.DEFAULTS:
        assert all(np.isfinite(sc.twin(prompts[i], sc.FIRST_MS, p).peak_to_mean) for i in range(4))      # guard 9: the far-bin mean exists


def test_the_scenes_are_shared_and_read_only():
    x = sc.refine_iq()
    assert x is sc.refine_iq() and not x.flags.writeable and x.shape == (2, sc.REFINE_SCENE_MS * sc.N)
    assert wm.init_u0(float(sc.refine_results()[2]["carrier_phase"])) == 0.0                              # the hair below zero
    assert [int(r["code_phase"]) for r in sc.refine_results()] == [0, sc.N - 1, sc.N // 3, sc.N // 2 + 1]
    r = sc.refine_results()[1]                                                                            # open loop: a shorter buffer's sums are a longer one's head
    alone = rm.open_loop_sums(x[1], sc.chips_pm(9), sc.FS, sc.N, float(r["doppler_hz"]), float(r["carrier_phase"]), int(r["code_phase"]), 41)
    assert alone.tobytes() == sc.model_sums(sc.RESIDUALS, 41)[1].tobytes()
