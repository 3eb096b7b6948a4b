"""numpy restatement of `grid_plan` (gypsum_amd/csrc/grid_plan.hpp): which cells kernel a flat search grid takes, with how many satellites
per wavefront and branch runs, its scratch and the size of its persistent grid.  Every argument may be an array (they broadcast); the
float64 expressions are written in the header's order.  tests/test_host_sanitizers.py::test_grid_plan compares the two over a sweep;
tests/test_gpu_grid_paths.py asks it which path a call must have taken.
"""
from __future__ import annotations

import numpy as np

FIELDS = ("path", "pipe", "waves", "gs", "parts", "wide_fold", "wgrid", "folded_bytes", "z_bytes", "partial_bytes")
CF_BYTES, PARTIAL_BYTES, CHIPS = 8, 24, 1023


def _ceil_div(a, b):
    return (a + b - 1) // b


def _plan_k(k: int, n_cus, n_units, n_sats, n_blk, no_pipe, no_shared_fwd, no_grid_fused, no_grid_parts, fused_waves):
    waves = np.where(fused_waves == 8, 8, 12)
    n_cells = n_units * n_sats
    fused = ((k <= 8) & (n_blk == 1) & (n_sats >= 4) & (n_sats <= 32) & (n_units >= n_cus * 16) & ~no_pipe & ~no_shared_fwd & ~no_grid_fused)
    slots = n_cus * np.where(waves == 8, 8.0, 12.0)
    cost = 2.0 * k * np.ceil(n_units.astype(np.float64) * n_sats / slots)
    gs_best, parts_best = np.ones_like(n_units), np.ones_like(n_units)
    for gs in (2, 4, 8, 16, 32):
        live = gs // 2 < n_sats            # the header's loop stops at the first gs with gs / 2 >= n_sats: every larger one fails it too
        groups = n_units.astype(np.float64) * _ceil_div(n_sats, gs)
        for pp in range(1, k + 1):
            if k % pp:
                continue
            t = (1.0 + gs) * (k // pp) * np.ceil(groups * pp / slots) + (0.25 * (1.0 + gs) if pp > 1 else 0.0)
            take = live & (t < cost * (0.97 if pp > 1 else 1.0))
            if pp > 1:
                take &= ~no_grid_parts
            cost = np.where(take, t, cost)
            gs_best = np.where(take, gs, gs_best)
            parts_best = np.where(take, pp, parts_best)
    shared = ~fused & (n_blk == 1) & (gs_best > 1) & ~no_pipe & ~no_shared_fwd
    rest = ~fused & ~shared
    pipe = rest & (n_blk == 1) & (k % 2 == 0) & ~no_pipe
    wave = rest & ~pipe & (n_blk == 1) & (k <= 8)
    path = np.select([fused, shared, pipe | wave], [1, 2, 3], 4)
    gs = np.where(shared, gs_best, 1)
    parts = np.where(shared, parts_best, 1)
    blocks_per_cu = 1 if k > 8 else 16 // k
    wgrid = np.select(
        [fused, shared, pipe, wave],
        [np.minimum(_ceil_div(n_units, waves), n_cus), np.minimum(_ceil_div(n_units * _ceil_div(n_sats, gs) * parts, waves), n_cus),
         np.minimum(_ceil_div(n_cells, 8), n_cus), np.minimum(_ceil_div(n_cells, 8), n_cus * 2)],
        np.minimum(n_cells, n_cus * blocks_per_cu) & ~7)
    zero = np.zeros_like(n_units)
    return {
        "path": path, "pipe": pipe.astype(np.int64), "waves": waves, "gs": gs, "parts": parts, "wide_fold": zero + (k > 8), "wgrid": np.maximum(1, wgrid),
        "folded_bytes": np.where(fused, 0, n_units * n_blk * k * 1024 * CF_BYTES),
        "z_bytes": np.where(fused, 0, n_units * n_blk * (k * CHIPS) * CF_BYTES) if k > 8 else zero,
        "partial_bytes": np.where(shared & (parts > 1), n_cells * parts * PARTIAL_BYTES, 0),
    }


def grid_plan(k, n_cus, n_units, n_sats, n_blk, no_pipe=False, no_shared_fwd=False, no_grid_fused=False, no_grid_parts=False, fused_waves=12):
    """{field: int64 array} over the broadcast of the arguments, FIELDS as GridPlan's members."""
    ints = np.broadcast_arrays(*[np.asarray(a, dtype=np.int64) for a in (k, n_cus, n_units, n_sats, n_blk, fused_waves)])
    flags = np.broadcast_arrays(*[np.asarray(a, dtype=bool) for a in (no_pipe, no_shared_fwd, no_grid_fused, no_grid_parts)], ints[0])[:4]
    shape = ints[0].shape
    ints, flags = [a.ravel() for a in ints], [a.ravel() for a in flags]
    out = {f: np.zeros(ints[0].size, dtype=np.int64) for f in FIELDS}
    for kk in np.unique(ints[0]):
        m = ints[0] == kk
        sub = _plan_k(int(kk), *[a[m] for a in ints[1:5]], *[a[m] for a in flags], ints[5][m])
        for f in FIELDS:
            out[f][m] = sub[f]
    return {f: v.reshape(shape) for f, v in out.items()}


def grid_plan_one(*args, **kwargs) -> dict:
    """The same for one shape, as plain ints."""
    return {f: int(v) for f, v in grid_plan(*args, **kwargs).items()}
