"""gyp_weak_refine and gyp_weak_measure across calls (the scenes of tests/weak_shapes_scene.py): 65 and 130 candidates -- a second and
a third workgroup of the plan kernels, the `i >= n_cand` guard, and the candidate-major decode of the sums kernels' grids -- each record
the bytes of that candidate alone; first_ms = 2^40 + 13, whose remainder by 20 is not the one its low 32 bits have, through the host
and the device forms; and 41 ms, 2000 ms, 41 ms again on one fresh context, with and without the caller's prompt and sums arrays, so
that every scratch row grows under a call and is then used by a smaller one.
"""
from __future__ import annotations

import numpy as np
import pytest

import weak_measure_model as mm
import weak_shapes_scene as sc
import weak_track_model as wm
from gypsum_amd import _lib, _records, engine
from gypsum_amd.engine import GypsumEngine

pytestmark = pytest.mark.gpu

COUNTS = (65, 130)


# ---------------------------------------------------------------------------------------------- candidate counts
@pytest.mark.parametrize("count", COUNTS)
def test_refine_records_of_many_candidates_are_those_of_each_alone(engine_factory, count):
    eng = engine_factory(sc.FS, sc.N)
    x = sc.head_of(sc.refine_iq(), 41)
    results = sc.many_results(count)
    rec, prompts = eng.refine_weak(x, 2, sc.FIRST_MS, results, want_prompts=True)
    assert np.count_nonzero(prompts) == count * 41
    for i in (0, 63, 64, count - 1):
        alone, p = eng.refine_weak(x, 2, sc.FIRST_MS, results[i:i + 1], want_prompts=True)
        assert alone.tobytes() == rec[i:i + 1].tobytes() and p.tobytes() == prompts[i:i + 1].tobytes(), i
        assert (int(alone[0]["stream"]), int(alone[0]["sat_id"])) == (int(results[i]["stream"]), int(results[i]["sat_id"]))
    known, known_p = eng.refine_weak(x, 2, sc.FIRST_MS, sc.refine_results(), want_prompts=True)      # the first four are the scene's candidates
    assert rec[:4].tobytes() == known.tobytes() and prompts[:4].tobytes() == known_p.tobytes()
    assert [int(r["edge"]) for r in rec[:4]] == [sc.refine_true_edge(i) for i in range(4)]


@pytest.mark.parametrize("count", COUNTS)
def test_measure_records_of_many_candidates_are_those_of_each_alone(engine_factory, count):
    eng = engine_factory(sc.FS, sc.N)
    x = sc.head_of(sc.refine_iq(), 41)
    refined = sc.many_refined(count)
    got = eng.measure_weak(x, 2, sc.FIRST_MS, refined, want_sums=True)
    assert all(np.count_nonzero(got[1][name]) == count * 2 * 41 for name in sc.SIX)
    assert [int(g) for g in got[0]["n_groups"]] == [mm.n_groups(41, sc.FIRST_MS, int(e)) for e in refined["edge"]]
    for i in (0, 63, 64, count - 1):
        alone = eng.measure_weak(x, 2, sc.FIRST_MS, refined[i:i + 1], want_sums=True)
        for a, g in zip(alone, got):
            assert a.tobytes() == g[i:i + 1].tobytes(), i
    if count == 65:                                     # every record, against the same candidates in reverse
        back = eng.measure_weak(x, 2, sc.FIRST_MS, refined[::-1], want_sums=True)
        for b, g in zip(back, got):
            assert np.ascontiguousarray(b[::-1]).tobytes() == g.tobytes()


# ---------------------------------------------------------------------------------------------- a large first_ms
def test_refine_at_a_first_ms_above_2_to_the_40(engine_factory):
    eng = engine_factory(sc.FS, sc.N)
    n_ms, big = 43, sc.BIG_FIRST_MS
    x = sc.head_of(sc.refine_iq(), n_ms)
    results = sc.refine_results()
    near, near_p = eng.refine_weak(x, 2, 13, results, want_prompts=True)
    far, far_p = eng.refine_weak(x, 2, big, results, want_prompts=True)
    assert far_p.tobytes() == near_p.tobytes()                                   # the prompts do not depend on first_ms
    for i, r in enumerate(results):
        for rec, first_ms in ((near[i], 13), (far[i], big)):
            sc.close_to(rec, sc.twin(far_p[i], first_ms, sc.DEFAULTS), float(r["doppler_hz"]), float(r["carrier_phase"]))
            assert int(rec["edge"]) == sc.refine_true_edge(i, first_ms)
        assert (int(far[i]["edge"]) - int(near[i]["edge"])) % 20 == (big - 13) % 20 == 16
        assert far[i]["delta_hz"] == near[i]["delta_hz"] and far[i]["carrier_phase"] == near[i]["carrier_phase"] and far[i]["edge_ratio"] == near[i]["edge_ratio"]
    # the device form
    d_iq = eng.alloc(x.nbytes).upload(x.reshape(-1))
    d_out, d_p = eng.alloc(4 * _lib.WEAK_REFINED.itemsize), eng.alloc(4 * n_ms * 8)
    try:
        eng.refine_weak_dev(d_iq.ptr.value, 2, n_ms * sc.N, big, n_ms, results, d_out.ptr.value, None, d_p.ptr.value)
        eng.sync()
        assert d_out.download(_lib.WEAK_REFINED, 4).tobytes() == far.tobytes()
        assert d_p.download(np.complex64, 4 * n_ms).tobytes() == far_p.tobytes()
    finally:
        for b in (d_iq, d_out, d_p):
            b.free()


def test_measure_at_a_first_ms_above_2_to_the_40(engine_factory):
    eng = engine_factory(sc.FS, sc.N)
    n_ms, big = 43, sc.BIG_FIRST_MS
    x = sc.head_of(sc.measure_iq(), n_ms)                                        # from the scene's first millisecond: the bit edges at index 0, 20, 40
    near = eng.measure_weak(x, 2, 13, sc.measure_refined(0, 13), want_sums=True)
    far = eng.measure_weak(x, 2, big, sc.measure_refined(0, big), want_sums=True)
    assert [int(e) for e in far[0]["edge"]] == [9] * 4 and [int(e) for e in near[0]["edge"]] == [13] * 4
    # head 0 under both: the same sums, W_m and folds, and records that differ in the edge alone
    for a, b in zip(near[1:], far[1:]):
        assert a.tobytes() == b.tobytes()
    same = far[0].copy()
    same["edge"] = 13
    assert same.tobytes() == near[0].tobytes() and np.all(far[0]["n_groups"] == 2) and np.all(far[0]["status"] == 0)
    # edges whose heads differ under the two first_ms: the sums are still the same bytes, the folds are the twin's given each first_ms
    edges = (13, 9, 0, 19)
    for first_ms in (13, big):
        refined = sc.measure_refined(0).copy()
        refined["edge"] = edges
        rec, sums, w, folds = eng.measure_weak(x, 2, first_ms, refined, want_sums=True)
        assert sums[:, 0].tobytes() == far[1][:, 0].tobytes() and w.tobytes() == far[2].tobytes()
        for i, r in enumerate(refined):
            c0 = wm.init_c0(int(r["code_phase"]), sc.N)
            for p in range(2):
                twin = engine.weak_measure_estimate(sums[i, p], w[i, p], first_ms, int(r["edge"]), c0, 1 << 39)
                for name in ("e_minus", "e_prompt", "e_plus", "wn", "dd", "c0", "n_groups", "status"):
                    assert folds[i, p][name] == twin[name], (first_ms, i, p, name)
                c0 = int(twin["c0"])
            assert int(rec[i]["n_groups"]) == mm.n_groups(n_ms, first_ms, int(r["edge"])) and int(rec[i]["c0"]) == c0
        assert [int(g) for g in rec["n_groups"]] == ([2, 1, 1, 1] if first_ms == 13 else [1, 2, 1, 1])
        if first_ms == big:                             # the device form
            d_iq = eng.alloc(x.nbytes).upload(x.reshape(-1))
            d_out, d_folds = eng.alloc(4 * _lib.WEAK_MEASURED.itemsize), eng.alloc(4 * 2 * _lib.WEAK_MEASURE_FOLD.itemsize)
            try:
                eng.measure_weak_dev(d_iq.ptr.value, 2, n_ms * sc.N, big, n_ms, refined, d_out.ptr.value, None, 0, 0, d_folds.ptr.value)
                eng.sync()
                assert d_out.download(_lib.WEAK_MEASURED, 4).tobytes() == rec.tobytes()
                assert d_folds.download(_lib.WEAK_MEASURE_FOLD, 8).tobytes() == folds.tobytes()
            finally:
                for b in (d_iq, d_out, d_folds):
                    b.free()


# ---------------------------------------------------------------------------------------------- scratch growth
def fresh_engine() -> GypsumEngine:
    eng = GypsumEngine(0)
    eng.set_stream_format(sc.FS, sc.N)
    return eng


def test_refine_small_large_small_on_one_context(engine_factory):
    x = sc.refine_iq()
    small, large = sc.head_of(x, 41), sc.head_of(x, 2000)
    results = sc.refine_results()
    known = engine_factory(sc.FS, sc.N).refine_weak(small, 2, sc.FIRST_MS, results, want_prompts=True)
    known_large = engine_factory(sc.FS, sc.N).refine_weak(large, 2, sc.FIRST_MS, results, want_prompts=True)
    # with the caller's prompts: stage_out, stage_iq, wref_plans and wref_power grow under the second call
    eng = fresh_engine()
    try:
        for buf, want in ((small, known), (large, known_large), (small, known)):
            rec, prompts = eng.refine_weak(buf, 2, sc.FIRST_MS, results, want_prompts=True)
            assert rec.tobytes() == want[0].tobytes() and prompts.tobytes() == want[1].tobytes(), buf.shape
    finally:
        eng.close()
    # without: the device form keeps the prompts in its scratch row, which grows too
    eng = fresh_engine()
    d_small, d_large = eng.alloc(small.nbytes).upload(small.reshape(-1)), eng.alloc(large.nbytes).upload(large.reshape(-1))
    d_out = eng.alloc(4 * _lib.WEAK_REFINED.itemsize)
    try:
        for d_iq, n_ms, want in ((d_small, 41, known), (d_large, 2000, known_large), (d_small, 41, known)):
            d_out.upload(np.zeros(4 * _lib.WEAK_REFINED.itemsize, dtype=np.uint8))
            eng.refine_weak_dev(d_iq.ptr.value, 2, n_ms * sc.N, sc.FIRST_MS, n_ms, results, d_out.ptr.value)
            eng.sync()
            assert d_out.download(_lib.WEAK_REFINED, 4).tobytes() == want[0].tobytes(), n_ms
    finally:
        for b in (d_small, d_large, d_out):
            b.free()
        eng.close()


def test_measure_small_large_small_on_one_context(engine_factory):
    x = sc.measure_iq()
    small, large = sc.head_of(x, 41), sc.head_of(x, 2000)
    refined = sc.measure_refined(0)
    prm = _records.WeakMeasureParams(spacing=1 << 39, passes=4)
    known = engine_factory(sc.FS, sc.N).measure_weak(small, 2, sc.FIRST_MS, refined, prm, want_sums=True)
    known_large = engine_factory(sc.FS, sc.N).measure_weak(large, 2, sc.FIRST_MS, refined, prm, want_sums=True)
    assert np.all(known[0]["n_groups"] == 2) and np.all(known_large[0]["n_groups"] == 100)
    for want_sums in (True, False):                     # without the caller's arrays the sums and the W_m live in scratch rows
        eng = fresh_engine()
        try:
            for buf, want in ((small, known), (large, known_large), (small, known)):
                got = eng.measure_weak(buf, 2, sc.FIRST_MS, refined, prm, want_sums=want_sums)
                assert got[0].tobytes() == want[0].tobytes(), (want_sums, buf.shape)
                if want_sums:
                    for g, w in zip(got[1:], want[1:]):
                        assert g.tobytes() == w.tobytes(), buf.shape
        finally:
            eng.close()
