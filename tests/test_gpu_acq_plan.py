"""What a search ran is what its plan said (csrc/acq_plan.hpp, restated by tests/acq_plan_model.py).

Every case searches 2 ms of synthetic signal -- three satellites planted per stream, close enough in Doppler that their grids overlap on
every coarse level -- for the satellites [31, 2, 17] and compares the library's witnesses with the model's plan: gyp_debug_get
"last_acq_lanes", "last_acq_levels" and "last_acq_shared_levels", and the per-level unit counters "last_acq_units_l<k>", which are
nonzero exactly on the levels the plan sends through the shared-forward kernels.  The records themselves are compared byte for byte
elsewhere (test_gpu_acq_lanes.py, test_gpu_acq_shared_fwd.py, test_gpu_acq_shared_edges.py, test_gpu_every_rate.py, test_gpu_parity.py);
this file only witnesses the path.
"""
from __future__ import annotations

import numpy as np
import pytest

import acq_plan_model as model
from gypsum_amd._lib import ACQ_RESULT, SYNTH_SAT, GypsumHipError, ptr

pytestmark = pytest.mark.gpu

FS_2, FS_8 = 2_046_000, 8_184_000
N_MS, MAX_STREAMS = 2, 5
SATS = [31, 2, 17]
SWITCH_DEFAULTS = {"acq_lanes": 2, "no_acq_split": 0, "no_acq_shared_fwd": 0}
NEW_NAMES = ("last_acq_lanes", "last_acq_levels", "last_acq_shared_levels")


class _Rig:
    """Five streams x 2 ms in device memory, made once per rate."""

    def __init__(self, eng, fs):
        self.eng, self.n = eng, fs // 1000
        rng = np.random.default_rng(4400 + self.n)
        scene = np.zeros((MAX_STREAMS, 3), dtype=SYNTH_SAT)
        for s in range(MAX_STREAMS):
            scene[s]["sat_id"] = SATS
            scene[s]["code_phase"] = rng.integers(0, self.n, 3)
            scene[s]["doppler_hz"] = 1000.0 + rng.uniform(-300, 300, 3)
            scene[s]["carrier_phase"] = rng.uniform(0, 2 * np.pi, 3)
            scene[s]["amplitude"] = 40.0 / self.n
            scene[s]["nav_bit_offset_ms"] = 5
        self.stride = N_MS * self.n
        self.iq = eng.alloc(MAX_STREAMS * self.stride * 8)
        eng.synth_iq(self.iq, MAX_STREAMS, self.stride, N_MS, scene, 40.0 / self.n, 44)
        self.out = eng.alloc(MAX_STREAMS * len(SATS) * ACQ_RESULT.itemsize)

    def free(self):
        self.iq.free()
        self.out.free()


@pytest.fixture(scope="module")
def rigs(engine_factory):
    made = {}

    def get(fs):
        if fs not in made:
            made[fs] = _Rig(engine_factory(fs, fs // 1000), fs)
        return made[fs]

    yield get
    for rig in made.values():
        rig.free()


def _witnessed(rig, switches, search):
    """`search(eng)` under `switches`: (the three new names, "last_acq_units_l<k>" for k = 1 .. 12)."""
    eng = rig.eng
    sw = dict(SWITCH_DEFAULTS, **switches)
    try:
        for name, value in sw.items():
            eng.debug_set(name, value)
        search(eng)
        units = [int(eng.debug_get(f"last_acq_units_l{k}")) for k in range(1, 13)]      # (waits for the search, helper contexts included)
        eng.sync()
        return tuple(int(eng.debug_get(name)) for name in NEW_NAMES), units
    finally:
        for name, value in SWITCH_DEFAULTS.items():
            eng.debug_set(name, value)


def _scan(rig, n_streams, **switches):
    sw = dict(SWITCH_DEFAULTS, **switches)
    plan = model.acq_plan(rig.n // 1023, rig.n, n_streams, len(SATS), N_MS, no_acq_shared_fwd=sw["no_acq_shared_fwd"], no_acq_split=sw["no_acq_split"],
                          acq_lanes=sw["acq_lanes"])
    names, units = _witnessed(rig, switches,
                              lambda eng: eng.acquire_dev(rig.iq.ptr.value, n_streams, rig.stride, N_MS, SATS, rig.out.ptr.value))
    return plan, names, units


def _assert_ran(plan, names, units):
    assert names == (plan["lanes"], plan["n_levels"], plan["shared_levels"])
    assert [u > 0 for u in units] == [k <= plan["shared_levels"] for k in range(1, 13)], units


@pytest.mark.parametrize("acq_lanes", [1, 2, 4])
@pytest.mark.parametrize("n_streams", [1, 4, 5])
def test_a_scan_ran_what_the_plan_said(rigs, n_streams, acq_lanes):
    plan, names, units = _scan(rigs(FS_8), n_streams, acq_lanes=acq_lanes)
    assert (plan["n_levels"], plan["shared_levels"]) == (10, 3)                       # the default parameters: 7000 Hz halved down to 13.67
    assert plan["lanes"] == {1: 1, 4: min(acq_lanes, 2), 5: min(acq_lanes, 2)}[n_streams]    # at least two streams per part
    assert sum(count for _, count in plan["parts"]) == n_streams
    _assert_ran(plan, names, units)


def test_an_unsplit_scan_is_one_lane(rigs):
    plan, names, units = _scan(rigs(FS_8), 4, no_acq_split=1)
    assert (plan["lanes"], plan["parts"]) == (1, [(0, 4)])
    _assert_ran(plan, names, units)


def test_a_scan_with_sharing_off_shares_no_level(rigs):
    plan, names, units = _scan(rigs(FS_8), 4, no_acq_shared_fwd=1)
    assert (plan["lanes"], plan["n_levels"], plan["shared_levels"], plan["max_units"]) == (2, 10, 0, 0)
    _assert_ran(plan, names, units)
    assert units == [0] * 12


def test_a_scan_at_two_samples_per_chip_shares_no_level(rigs):
    plan, names, units = _scan(rigs(FS_2), 4)
    assert (plan["lanes"], plan["n_levels"], plan["shared_levels"]) == (2, 10, 0)
    _assert_ran(plan, names, units)


def test_a_single_level_is_one_level_on_one_lane(rigs):
    rig = rigs(FS_8)
    plan = model.acq_plan(8, rig.n, 4, len(SATS), N_MS, spread0=1750.0, single_level=1, no_acq_split=1)      # (only a scan is split)
    assert (plan["lanes"], plan["n_levels"], plan["shared_levels"]) == (1, 1, 1)
    ids = np.array(SATS, dtype=np.int32)
    names, units = _witnessed(rig, {}, lambda eng: eng._check(eng.lib.gyp_search_level_dev(eng.ctx, rig.iq.ptr, 4, rig.stride, N_MS, ptr(ids), len(SATS), 0.0, 1750.0,
                                                                                             rig.out.ptr)))
    _assert_ran(plan, names, units)


def test_the_new_names_are_read_only(rigs):
    eng = rigs(FS_8).eng
    _scan(rigs(FS_8), 4)
    before = [eng.debug_get(name) for name in NEW_NAMES]
    assert before == [2.0, 10.0, 3.0]
    for name in NEW_NAMES:
        with pytest.raises(GypsumHipError):
            eng.debug_set(name, 1)
    assert [eng.debug_get(name) for name in NEW_NAMES] == before
