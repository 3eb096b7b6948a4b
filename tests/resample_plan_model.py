"""Python restatement of what the sample path launches (gypsum_amd/csrc/resample_plan.hpp): the ratio of the two rates and
resample_kernel's tiling of the output -- whole periods per tile or one period cut into phase chunks, the LDS reserved, the grid and
whether it fits.  Written from the host code as it stood before the header existed (resample_cached_design's n_in, n_out, g, L, M;
resample_shape's two branches and its "launch too large" refusal), with one difference the invariant below asked for: a budget below
the tap count, which no caller can pass (the debug switch starts at 1024), reserves T samples and not the budget.  Every argument of
resample_tilings may be an array (they broadcast).  tests/test_host_sanitizers.py::test_resample_plan compares the two over a sweep
and checks tile_span against the LDS of every plan.
"""
from __future__ import annotations

import numpy as np

INT32_MAX = 2 ** 31 - 1
MAX_GRID_Y = 65535
RATIO_FIELDS = ("n_in", "n_out", "g", "L", "M")
FIELDS = ("fits", "n_tiles", "lds_samples", "p_first", "n_periods", "np_tile", "pc_tile", "n_pchunks")


def resample_ratio(fs_in, fs_out) -> dict:
    """n_in, n_out (kHz), g = gcd, L = n_out / g outputs and M = n_in / g inputs per period; arrays broadcast."""
    n_in, n_out = np.broadcast_arrays(np.asarray(fs_in, dtype=np.int64) // 1000, np.asarray(fs_out, dtype=np.int64) // 1000)
    g = np.gcd(n_in, n_out)
    return {"n_in": n_in, "n_out": n_out, "g": g, "L": n_out // g, "M": n_in // g}


def resample_tilings(n_in, n_out, taps, n_streams, first_ms, n_ms, tile_samples) -> np.ndarray:
    """int64 [rows, len(FIELDS)] over the broadcast of the arguments (rates in kHz, n_ms >= 1)."""
    cols = [c.ravel() for c in np.broadcast_arrays(*[np.asarray(a, dtype=np.int64) for a in (n_in, n_out, taps, n_streams, first_ms, n_ms, tile_samples)])]
    n_in, n_out, T, n_streams, first_ms, n_ms, TS = cols
    g = np.gcd(n_in, n_out)
    L, M = n_out // g, n_in // g
    n_periods = n_ms * g
    whole = M + T - 1 <= TS
    # whole periods: as many as fit the budget, never more than there are
    np_tile = np.where(whole, np.minimum(np.maximum(1, (TS - T + 1) // M), n_periods), 1)
    # one period in phase chunks: (TS - T - 1) * L / M phases, at least one (C++ truncates, Python floors: both are below 1 when negative)
    pc_tile = np.where(whole, L, np.maximum(1, (TS - T - 1) * L // M))
    n_pchunks = -(-L // pc_tile)
    lds = np.where(whole, np_tile * M + T - 1, np.maximum(TS, T))
    n_tiles = -(-n_periods // np_tile) * n_pchunks
    fits = (n_tiles <= INT32_MAX) & (n_streams <= MAX_GRID_Y)
    out = np.stack([fits.astype(np.int64), n_tiles, lds, first_ms * g, n_periods, np_tile, pc_tile, n_pchunks], axis=1)
    out[~fits] = 0                                       # a launch that does not fit is refused: nothing else is planned
    return out


def tile_span(plan: dict, L, M, T, tile_index):
    """The input samples resample_kernel stages for tile `tile_index` (its blockIdx.x) of a plan, by the kernel's own arithmetic
    (kernels_resample.hpp, resample_kernel: `chunk`, `ptile`, `P0`, `P1`, `pa`, `pb`, `off_a`, `off_b` and
    `span = (P1 - 1 - P0) * M + off_b - off_a + T`, with off(p) = p * M // L).  `plan` maps FIELDS to arrays; everything broadcasts."""
    tile_index = np.asarray(tile_index, dtype=np.int64)
    chunk, ptile = tile_index % plan["n_pchunks"], tile_index // plan["n_pchunks"]
    end = plan["p_first"] + plan["n_periods"]
    P0 = plan["p_first"] + ptile * plan["np_tile"]
    P1 = np.minimum(P0 + plan["np_tile"], end)
    pa = chunk * plan["pc_tile"]
    pb = np.minimum(pa + plan["pc_tile"], L)
    return (P1 - 1 - P0) * M + (pb - 1) * M // L - pa * M // L + T


def mixer_params(fs: int, f_hz: int):
    """(f mod fs in [0, fs), 4 / fs, 1 / (2 fs)) in Python integers and float64."""
    return f_hz % fs, 4.0 / float(fs), 0.5 / float(fs)
