"""Python restatement of what a search runs (gypsum_amd/csrc/acq_plan.hpp): whether it fits, its levels and how many of them share
forward transforms, the room for shared-forward units, the elements of every acq_* scratch buffer, the grids of the bookkeeping
launches and the parts a multi-stream scan goes through in.  Written from the host code as it stood before the header existed
(acquire_search's reservations, level loop and launches; gyp_acquire_dev's lanes).  Every argument of acq_plans may be an array (they
broadcast).  tests/test_host_sanitizers.py::test_acq_plan compares the two over a sweep; tests/test_gpu_acq_plan.py asks it what a
search must have run; acq_units_model.max_units_for is a call into it.
"""
from __future__ import annotations

import numpy as np

MAX_BINS = 28                # kMaxBins
SPEC_UNIT_BYTES = 131072     # one unit-millisecond of spectra: 8 branches x 2048 complex64 (kSpecUnitMs * sizeof(cf))
MAX_LANES = 4                # kMaxAcqLanes
INT32_MAX = 2 ** 31 - 1
FIELDS = ("fits", "n_states", "n_cells", "n_levels", "shared_levels", "bins_per_spread_bits", "max_units", "states", "cells", "out", "refined",
          "partial64", "profiles", "spectra", "tpb", "nblk", "refine_x", "refine_y", "exact_z", "lanes",
          *(f"lane_first{i}" for i in range(MAX_LANES)), *(f"lane_streams{i}" for i in range(MAX_LANES)))


def level_spreads(spread0: float, single_level: bool, min_spread: float) -> list[float]:
    """The spreads of a search's levels: halved while they are at least min_spread (acquisition.py:81,89), or the one asked for."""
    if single_level:
        return [spread0]
    spreads, spread = [], spread0
    while spread >= min_spread:
        spreads.append(spread)
        spread /= 2.0
    return spreads


def acq_plans(k, n, n_streams, n_sats, n_ms, spread0=7000.0, single_level=0, initial_spread=7000.0, min_spread=10.0, bins_per_spread=10.0,
              no_pipe=0, no_acq_shared_fwd=0, no_acq_split=0, is_helper=0, acq_lanes=2) -> np.ndarray:
    """int64 [rows, len(FIELDS)] over the broadcast of the arguments (bins_per_spread as the bits of the float64)."""
    ints = [np.asarray(a, dtype=np.int64) for a in (k, n, n_streams, n_sats, n_ms, single_level, no_pipe, no_acq_shared_fwd, no_acq_split, is_helper, acq_lanes)]
    reals = [np.asarray(a, dtype=np.float64) for a in (spread0, initial_spread, min_spread, bins_per_spread)]
    cols = [c.ravel() for c in np.broadcast_arrays(*ints, *reals)]
    k, n, n_streams, n_sats, n_ms, single, no_pipe, no_shared, no_split, helper, acq_lanes = cols[:11]
    spread0, initial, min_spread, bps = cols[11:]
    f = {name: np.zeros(k.size, dtype=np.int64) for name in FIELDS}
    n_states = n_streams * n_sats
    n_cells = n_states * MAX_BINS
    fits = (n_cells <= INT32_MAX) & (n_ms <= 65535)      # int32 cell indices; acq_refine_kernel's grid has n_ms rows of blocks
    f["fits"], f["n_states"], f["n_cells"] = fits, n_states, n_cells
    f["bins_per_spread_bits"] = bps.copy().view(np.int64)
    # room of the spectra buffer: 3 * 28 units per stream, 1 GiB at most, never more than there are cells; K = 8 on the pipelined path only
    can_share = (k == 8) & (no_pipe == 0) & (no_shared == 0)
    f["max_units"] = np.where(can_share, np.minimum(n_cells, np.minimum(2 ** 30 // (np.maximum(n_ms, 1) * SPEC_UNIT_BYTES), n_streams * 3 * MAX_BINS)), 0)
    # levels, and the leading ones on which every satellite of a stream still has the same bins (spread * 4 >= the initial spread)
    keys = np.stack([spread0, single.astype(np.float64), min_spread, initial], axis=1)
    for key in np.unique(keys, axis=0):
        spreads = level_spreads(key[0], key[1] != 0, key[2])
        rows = (keys == key).all(axis=1)
        f["n_levels"][rows] = len(spreads)
        f["shared_levels"][rows] = sum(1 for s in spreads if s * 4.0 >= key[3])
    f["shared_levels"] = np.where(f["max_units"] > 0, f["shared_levels"], 0)
    f["states"] = n_states
    f["cells"] = f["out"] = f["refined"] = n_cells
    f["partial64"] = n_cells * n_ms
    f["profiles"] = n_states * 2 * n
    f["spectra"] = f["max_units"] * n_ms * (SPEC_UNIT_BYTES // 8)
    f["tpb"] = np.full(k.size, 64)
    f["nblk"] = -(-n_states // 64)
    f["refine_x"] = np.minimum(n_cells, 2 * n_states)
    f["refine_y"] = n_ms
    f["exact_z"] = np.minimum(n_states, 32)
    # parts of a scan: at least two streams each, the remaining streams spread evenly over the remaining parts
    lanes = np.where((helper != 0) | (no_split != 0), 1, np.maximum(1, np.minimum(np.minimum(acq_lanes, n_streams // 2), MAX_LANES)))
    f["lanes"] = lanes
    first = np.zeros(k.size, dtype=np.int64)
    for i in range(MAX_LANES):
        on = i < lanes
        count = np.where(on, (n_streams - first) // np.maximum(lanes - i, 1), 0)
        f[f"lane_first{i}"], f[f"lane_streams{i}"] = np.where(on, first, 0), count
        first = first + count
    out = np.stack([np.asarray(f[name], dtype=np.int64) for name in FIELDS], axis=1)
    out[~fits] = 0                                       # a search that does not fit is refused: nothing else is planned
    return out


def acq_plan(*args, **kwargs) -> dict:
    """The same for one shape, as plain ints, with the parts' (first stream, streams) under "parts"."""
    row = dict(zip(FIELDS, acq_plans(*args, **kwargs)[0].tolist()))
    row["parts"] = [(row[f"lane_first{i}"], row[f"lane_streams{i}"]) for i in range(row["lanes"])]
    return row
