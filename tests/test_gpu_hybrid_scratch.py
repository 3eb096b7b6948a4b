"""The hybrid search's scratch members belong to it alone: a hybrid grid, then gyp_acquire (which reserves and fills the acq_* members,
partial64 and the staging buffers), then the same grid again on ONE engine -- the two grids are bit-identical to each other and to
a fresh engine's, and so are the weak-signal search's records taken before and after."""
from __future__ import annotations

import numpy as np
import pytest

import hybrid_model as hm
from gypsum_amd import synth
from gypsum_amd.engine import GypsumEngine

pytestmark = pytest.mark.gpu

FS, N = 2_046_000, 2046
T, M, FLAGS = 4, 5, hm.ALTERNATE | hm.CODE_DOPPLER
SATS = (2, 9, 17, 30)
BINS = tuple(-2000.0 + 500.0 * i for i in range(9))


def test_grids_around_an_acquisition_are_the_same_bits():
    scene = synth.random_scene(FS, T * M, 3, 20261020, max_doppler=2500.0)
    x = hm.render(scene, code_doppler=True)
    ids = [s.sat_id for s in scene.sats]
    eng, fresh = GypsumEngine(0), GypsumEngine(0)
    try:
        eng.set_stream_format(FS, N)
        fresh.set_stream_format(FS, N)
        first = eng.correlate_grid_hybrid(x, 1, T, M, FLAGS, SATS + tuple(ids), BINS)
        weak_first = eng.acquire_weak(x, 1, T, M, FLAGS, ids, 0.0, 3000.0, 25.0)
        acq = eng.acquire(x[:10 * N], 1, 10, list(range(1, 33)))
        again = eng.correlate_grid_hybrid(x, 1, T, M, FLAGS, SATS + tuple(ids), BINS)
        weak_again = eng.acquire_weak(x, 1, T, M, FLAGS, ids, 0.0, 3000.0, 25.0)
        alone = fresh.correlate_grid_hybrid(x, 1, T, M, FLAGS, SATS + tuple(ids), BINS)
        weak_alone = fresh.acquire_weak(x, 1, T, M, FLAGS, ids, 0.0, 3000.0, 25.0)
        acq_alone = fresh.acquire(x[:10 * N], 1, 10, list(range(1, 33)))
    finally:
        eng.close()
        fresh.close()
    assert np.isfinite(first["peak"]).all() and (first["peak"] > 0).all() and (first["n_off"] == N - 5).all()
    assert first.tobytes() == again.tobytes() == alone.tobytes()
    assert weak_first.tobytes() == weak_again.tobytes() == weak_alone.tobytes()
    assert acq.tobytes() == acq_alone.tobytes()          # and the acquisition is not disturbed by the hybrid calls before it
    by_sat = {int(r["sat_id"]): r for r in weak_first}
    for s in scene.sats:                                 # the search did find what the scene holds (default amplitudes: strong)
        assert abs(float(by_sat[s.sat_id]["doppler_hz"]) - s.doppler_hz) <= 25.0 and int(by_sat[s.sat_id]["code_phase"]) == s.code_phase
