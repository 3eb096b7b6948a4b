"""Every launch branch of a flat grid (launch_grid, csrc/gypsum_hip.hip) off the fused kernel, on grids of a few cells: the path taken is
the one tests/grid_plan_model.py plans for the device's CU count, and the records agree with the per-cell entry point on the same samples
to the bar tests/test_gpu_parity.py holds the shared-forward and workgroup-per-cell kernels to.  (The fused kernel needs 16 units per CU:
tests/test_gpu_grid_shapes.py::test_fused_grid_kernel_against_folded_rows_and_oracle.)"""
import functools
import re

import numpy as np
import pytest

import grid_plan_model
from gypsum_amd._lib import CELL_DESC, GYP_NON_COHERENT

pytestmark = pytest.mark.gpu

DOPPLER_EXTRA = [-1500.0, 250.0]
# (samples per chip, satellites, ms, switches) -> (path, pipe (path 3), parts (path 2))
CASES = [
    ((2, 1, 1, ()), (3, 1, 1)),
    ((2, 1, 1, ("no_pipe",)), (3, 0, 1)),
    ((2, 11, 1, ("no_shared_fwd",)), (3, 1, 1)),
    ((5, 1, 1, ()), (3, 0, 1)),
    ((16, 1, 1, ()), (3, 1, 1)),
    ((16, 1, 1, ("no_pipe",)), (4, 0, 1)),
    ((16, 11, 1, ()), (2, 0, 16)),
    ((16, 11, 1, ("no_grid_parts",)), (3, 1, 1)),     # whole units per item cost more than a wavefront per cell
    ((2, 3, 2, ()), (4, 0, 1)),                     # non-coherent, two blocks
]


@functools.lru_cache(maxsize=None)
def scene_streams(fs: int):
    """Two streams of 3 ms (the second is the first conjugated and reversed), the planted satellites and 3 Doppler bins."""
    from gypsum_amd import synth

    n = fs // 1000
    scene = synth.random_scene(fs, 3, 3, 1234 + n, max_doppler=6000.0, with_nav_bits=False)
    iq = synth.render(scene)
    iq2 = np.concatenate([iq, np.conj(iq[::-1])]).astype(np.complex64)
    planted = [s.sat_id for s in scene.sats]
    return iq2, planted, [float(round(scene.sats[0].doppler_hz))] + DOPPLER_EXTRA


@pytest.fixture(scope="module")
def per_cell():
    """The per-cell entry point's records, once per (rate, satellites, ms)."""
    return {}


@pytest.mark.parametrize("case,expected", CASES, ids=[f"k{c[0]}-{c[1]}sats-{c[2]}ms" + "".join("-" + s for s in c[3]) for c, _ in CASES])
def test_grid_path_agrees_with_per_cell_entry_point(engine_factory, per_cell, case, expected):
    k, n_sats, n_ms, switches = case
    fs, n = k * 1_023_000, k * 1023
    eng = engine_factory(fs, n)
    iq2, planted, dopp = scene_streams(fs)
    sats = planted + [sv for sv in (1, 5, 9, 13, 17, 21, 25, 29, 31, 32, 2) if sv not in planted]
    sats = sats[:n_sats]
    two = np.concatenate([iq2[:n_ms * n], iq2[3 * n:(3 + n_ms) * n]])
    if (k, n_sats, n_ms) not in per_cell:
        cells = np.zeros((2, n_sats, len(dopp)), dtype=CELL_DESC)
        cells["stream"] = np.arange(2)[:, None, None]
        cells["sat_id"] = np.array(sats)[None, :, None]
        cells["doppler_hz"] = np.array(dopp)[None, None, :]
        cells["tap_index"] = -1
        c, _ = eng.correlate_cells(two, 2, n_ms, cells.reshape(-1), GYP_NON_COHERENT)
        c = c.reshape(cells.shape)
        c.setflags(write=False)
        per_cell[k, n_sats, n_ms] = c
    c = per_cell[k, n_sats, n_ms]
    n_cus = int(re.search(r"(\d+) CUs\)$", eng.device_name()).group(1))      # the count the library plans with (no torch in this process: it brings a second ROCm stack)
    want = grid_plan_model.grid_plan_one(k, n_cus, 2 * len(dopp), n_sats, n_ms, **{s: True for s in switches})
    assert (want["path"], want["pipe"], want["parts"]) == expected
    try:
        for s in switches:
            eng.debug_set(s, 1)
        g = eng.correlate_grid(two, 2, n_ms, sats, dopp, GYP_NON_COHERENT)
        path = int(eng.debug_get("last_grid_path"))
    finally:
        for s in switches:
            eng.debug_set(s, 0)
    assert path == want["path"]
    assert np.array_equal(g["argmax"], c["argmax"])
    assert np.array_equal(g["n_max"], c["n_max"])
    for f in ("peak", "sum"):
        print(f"{f}: largest relative difference {np.max(np.abs(g[f] / c[f] - 1.0)):.3g}")
        np.testing.assert_allclose(g[f], c[f], rtol=3e-6)
