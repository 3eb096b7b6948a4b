"""CPU model of the shared-forward planner of the acquisition search (acq_compact_units_kernel, kernels_acq.hpp; the model itself
is tests/acq_units_model.py, which the GPU tests hold the device's counters against): the level's
active cells (acq_plan_kernel's bins, minus the bins whose records the previous level already holds) grouped by exact
(stream, Doppler) equality; a unit of two or more cells gets one forward pass, units are numbered in the order of their first cell
and those beyond the spectra buffer's room stay on the unshared kernel.  Checked here: how many distinct bins the first three levels
of a scan put on the shared grids for given winners, and that every active cell lands in exactly one of the two work lists."""
from __future__ import annotations

import numpy as np
import pytest

from acq_units_model import MAX_BINS, N_SATS, _check_partition, expected_counts, level_bins, max_units_for, plan_level, plan_units


def _scan_levels(winners_1, winners_2, n_streams):
    """Levels 1-3 of a scan for given level-1 and level-2 winners (offsets in bins of their level)."""
    c1 = np.zeros((n_streams, N_SATS))
    l1 = plan_level(c1, 7000.0, None)
    bins1 = [level_bins(0.0, 7000.0)] * (n_streams * N_SATS)
    c2 = np.array([[bins1[0][w] for w in row] for row in winners_1], dtype=float)
    l2 = plan_level(c2, 3500.0, bins1)
    bins2 = [level_bins(c2[s, k], 3500.0) for s in range(n_streams) for k in range(N_SATS)]
    c3 = np.array([[bins2[s * N_SATS + k][winners_2[s][k]] for k in range(N_SATS)] for s in range(n_streams)], dtype=float)
    l3 = plan_level(c3, 1750.0, bins2)
    return l1, l2, l3


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_first_three_levels_fall_on_shared_grids(seed):
    rng = np.random.default_rng(seed)
    n_streams = 6
    w1 = rng.integers(0, 20, (n_streams, N_SATS))
    w2 = rng.integers(0, 20, (n_streams, N_SATS))
    l1, l2, l3 = _scan_levels(w1, w2, n_streams)
    # level 2: the multiples of 350 Hz in [-10500, 9450] that level 1 did not evaluate (58 - 20); level 3: multiples of 175 Hz
    for lvl, cells, bound in ((1, l1, 20), (2, l2, 38), (3, l3, 134)):
        units, sh_cell, sh_unit, order = plan_units(cells, max_units=10**6)
        _check_partition(cells, units, sh_cell, sh_unit, order)
        for s in range(n_streams):
            dops = {d for (st, d, on) in cells if on and st == s}
            assert len(dops) <= bound, (lvl, s, len(dops))
            step = {1: 700, 2: 350, 3: 175}[lvl]
            assert all(d % step == 0 for d in dops)
        if lvl == 1:
            assert len(units) == 20 * n_streams and not order          # every level-1 cell shares its bin with 31 others
            assert len(sh_cell) == 20 * N_SATS * n_streams
        if lvl == 2:   # inside level 1's range only the odd multiples of 350 Hz are new: the even ones are level 1's records
            assert all((d // 350) % 2 != 0 or not -7000 <= d <= 6300 for (_, d, on) in cells if on)


def test_level_2_distinct_bins_for_given_winners():
    """Half the satellites of a stream won at 0 Hz (bin 10), half at -7000 Hz (bin 0): level 2's new cells fall on 10 + 15 bins."""
    w1 = np.array([[10] * 16 + [0] * 16])
    _, l2, _ = _scan_levels(w1, np.zeros((1, N_SATS), dtype=int), 1)
    units, sh_cell, sh_unit, order = plan_units(l2, max_units=10**6)
    _check_partition(l2, units, sh_cell, sh_unit, order)
    around_0 = [d for d in range(-3500, 3500, 350) if d % 700]                          # the odd multiples of 350
    around_m7000 = [d for d in range(-10500, -3500, 350) if d < -7000 or d % 700]       # below level 1's range, all new
    assert len(units) == 25 and not order
    assert sorted(l2[u][1] for u in units) == sorted(around_0 + around_m7000)
    assert len(sh_cell) == 16 * 10 + 16 * 15


def test_units_beyond_the_room_stay_unshared():
    l1, _, _ = _scan_levels(np.zeros((3, N_SATS), dtype=int), np.zeros((3, N_SATS), dtype=int), 3)
    for cap in (0, 1, 19, 20, 21, 59, 60):
        units, sh_cell, sh_unit, order = plan_units(l1, max_units=cap)
        _check_partition(l1, units, sh_cell, sh_unit, order)
        assert len(units) == min(cap, 60)
        assert len(order) == (60 - len(units)) * N_SATS


def test_one_satellite_shares_nothing():
    cells = plan_level(np.zeros((2, N_SATS)), 7000.0, None)
    cells = [(s, d, on and (i % (N_SATS * MAX_BINS)) < MAX_BINS) for i, (s, d, on) in enumerate(cells)]   # satellite 0 of each stream only
    units, sh_cell, sh_unit, order = plan_units(cells, max_units=10**6)
    _check_partition(cells, units, sh_cell, sh_unit, order)
    assert not units and len(order) == 2 * 20


def test_expected_counts_on_the_hand_cases():
    """expected_counts (what gyp_debug_get "last_acq_units" / "last_acq_shared_cells" / "last_acq_unshared_cells" are held against) on
    the three cases counted by hand above, and the room for units as acquire_search computes it."""
    for n_streams in (1, 6, 13):
        z = np.zeros((n_streams, N_SATS), dtype=int)
        l1, _, _ = _scan_levels(z, z, n_streams)
        assert expected_counts([l1], max_units=10**6) == (20 * n_streams, 20 * N_SATS * n_streams, 0)
    _, l2, _ = _scan_levels(np.array([[10] * 16 + [0] * 16]), np.zeros((1, N_SATS), dtype=int), 1)
    assert expected_counts([l2], max_units=10**6) == (25, 16 * 10 + 16 * 15, 0)
    z = np.zeros((3, N_SATS), dtype=int)
    l1, _, _ = _scan_levels(z, z, 3)
    for cap in (0, 1, 19, 20, 21, 59, 60):
        assert expected_counts([l1], max_units=cap) == (min(cap, 60), min(cap, 60) * N_SATS, (60 - min(cap, 60)) * N_SATS)
    assert expected_counts([l1, l2], max_units=10**6) == (60 + 25, 60 * N_SATS + 400, 0)     # summed over the levels given
    # the room: 84 units per stream, 1 GiB of spectra at most, never more than there are cells
    assert max_units_for(13, 32, 10) == 819 and max_units_for(2, 32, 10) == 168 and max_units_for(7, 32, 10) == 588
    assert max_units_for(12, 32, 40) == 204 and max_units_for(6, 32, 40) == 204
    assert max_units_for(1, 2, 1) == 56 and max_units_for(1, 1, 10) == 28
