"""CPU model of the shared-forward planner of the acquisition search (acq_plan_kernel and acq_compact_units_kernel,
kernels_acq.hpp; the room for units is acq_plan_model's, the restatement of acq_plan.hpp): the level's active cells -- the level's bins,
minus the bins whose records the previous level already holds -- grouped by exact (stream, Doppler) equality; a unit of two or more
cells gets one forward pass, units are numbered in the order of their first cell and those beyond the spectra buffer's room stay on
the unshared kernel.  Plain Python over lists: the CPU tests check it against hand counts (test_acq_units_plan.py), the GPU tests
check the device's counters against it (test_gpu_acq_shared_edges.py)."""
from __future__ import annotations

import numpy as np

import acq_plan_model

MAX_BINS = 28           # kMaxBins
N_SATS = 32


def level_bins(center: float, spread: float, bins_per_spread: float = 10.0) -> list[int]:
    """acq_plan_kernel: range(int(c - s), int(c + s), int(s / 10))."""
    lo, hi, step = int(center - spread), int(center + spread), int(spread / bins_per_spread)
    return list(range(lo, hi, step))[:MAX_BINS]


def plan_level(centers: np.ndarray, spread: float, prev: list[list[int]] | None, bins_per_spread: float = 10.0, reuse: bool = True):
    """Cells [state][28] of one level: (stream, doppler, active), state = stream * n_sats + satellite for centers[n_streams, n_sats].
    A bin the previous level evaluated (`prev`: its bins per state) is not active -- record reuse; with `reuse` off
    (gyp_params::acq_reuse_level_records = 0) no bin is inactive."""
    n_streams, n_sats = centers.shape
    cells = []
    for s in range(n_streams):
        for sat in range(n_sats):
            bins = level_bins(centers[s, sat], spread, bins_per_spread)
            done = set(prev[s * n_sats + sat]) if prev is not None and reuse else set()
            for b in range(MAX_BINS):
                cells.append((s, bins[b] if b < len(bins) else 0, b < len(bins) and bins[b] not in done))
    return cells


def plan_units(cells, max_units: int, n_sats: int = N_SATS):
    """The kernel's lists: units (first cell of each), the shared cells unit after unit with their unit, the unshared cells ascending."""
    per_stream = n_sats * MAX_BINS
    units, sh_cell, sh_unit, order = [], [], [], []
    for s0 in range(0, len(cells), per_stream):
        members: dict[int, list[int]] = {}
        for c in range(s0, s0 + per_stream):
            if cells[c][2]:
                members.setdefault(cells[c][1], []).append(c)
        shared = set()
        for dop, cs in sorted(members.items(), key=lambda kv: kv[1][0]):   # units in the order of their first cell
            if len(cs) >= 2 and len(units) < max_units:
                u = len(units)
                units.append(cs[0])
                sh_cell += cs
                sh_unit += [u] * len(cs)
                shared.update(cs)
        order += [c for c in range(s0, s0 + per_stream) if cells[c][2] and c not in shared]
    return units, sh_cell, sh_unit, order


def _check_partition(cells, units, sh_cell, sh_unit, order):
    active = [c for c, (_, _, on) in enumerate(cells) if on]
    assert sorted(sh_cell + order) == active                       # nothing lost, nothing twice
    assert order == sorted(order)
    for c, u in zip(sh_cell, sh_unit):                             # a cell reads the spectra of its own (stream, Doppler)
        assert cells[c][:2] == cells[units[u]][:2]
    assert all(np.diff(sh_unit) >= 0)                              # grouped: a unit's consumers are neighbours in the list


def max_units_for(n_streams: int, n_sats: int, n_ms: int) -> int:
    """Units the spectra buffer of a search of n_streams x n_sats states over n_ms milliseconds has room for (acq_plan.hpp, restated
    in acq_plan_model.py): 3 * 28 = 84 per stream, 1 GiB at most, never more than there are cells."""
    return acq_plan_model.acq_plan(8, 8184, n_streams, n_sats, n_ms)["max_units"]


def expected_counts(levels, max_units: int, n_sats: int = N_SATS):
    """(units, shared cells, unshared cells) summed over `levels`, each a list of cells as plan_level gives it and searched with
    shared forward transforms in a buffer with room for `max_units` units: what gyp_debug_get "last_acq_units" /
    "last_acq_shared_cells" / "last_acq_unshared_cells" report after those levels."""
    n_units = n_shared = n_unshared = 0
    for cells in levels:
        units, sh_cell, sh_unit, order = plan_units(cells, max_units, n_sats)
        _check_partition(cells, units, sh_cell, sh_unit, order)
        n_units += len(units)
        n_shared += len(sh_cell)
        n_unshared += len(order)
    return n_units, n_shared, n_unshared


def active_cells(cells) -> int:
    """Cells of a level that are correlated at all: every one of them is on the unshared list where nothing is shared."""
    return sum(1 for _, _, on in cells if on)


def scan_levels(winners, n_streams: int, n_sats: int, initial_spread: float = 7000.0, min_spread: float = 10.0,
                bins_per_spread: float = 10.0, reuse: bool = True):
    """The levels of a whole scan as lists of cells, for given level winners: winners[state] = the Doppler bin each level of that
    state's search ended on (the float64 oracle's trace), state = stream * n_sats + satellite.  Level i is centred on level i - 1's
    winner (acquisition.py:81-89)."""
    levels = []
    prev = None
    spread, i = initial_spread, 0
    while spread >= min_spread:
        centers = np.array([[0.0 if i == 0 else float(winners[s * n_sats + k][i - 1]) for k in range(n_sats)] for s in range(n_streams)])
        levels.append(plan_level(centers, spread, prev, bins_per_spread, reuse))
        prev = [level_bins(centers[s, k], spread, bins_per_spread) for s in range(n_streams) for k in range(n_sats)]
        spread /= 2.0
        i += 1
    return levels


def expected_scan_counts(winners, n_streams: int, n_sats: int, n_ms: int, shared: bool = True, initial_spread: float = 7000.0,
                         min_spread: float = 10.0, bins_per_spread: float = 10.0, reuse: bool = True):
    """The three counters after a whole scan on ONE context: levels 1-3 through the unit planner (spread * 4 >= the initial spread),
    every active cell of the finer levels -- and of all levels with the switch off -- on the unshared list."""
    levels = scan_levels(winners, n_streams, n_sats, initial_spread, min_spread, bins_per_spread, reuse)
    n_coarse = min(3, len(levels)) if shared else 0
    u, sh, un = expected_counts(levels[:n_coarse], max_units_for(n_streams, n_sats, n_ms), n_sats)
    return u, sh, un + sum(active_cells(c) for c in levels[n_coarse:])
