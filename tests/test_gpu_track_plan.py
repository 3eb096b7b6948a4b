"""What a gyp_track_block_dev call ran is what its plan said (csrc/track_plan.hpp, restated by tests/track_plan_model.py).

Every case tracks one block of synthetic signal and compares the library's witnesses with the model's plan for the device's CU count:
gyp_debug_get "last_track_flow"; for the speculative flows the first two values of gyp_debug_spec_redo_read (sub-blocks, and rounds
under the round protocol or sub-blocks again in the r03 form); for the throughput kernel "last_exact_path" and the launch count of
gyp_debug_track_timing.  The records themselves are compared with the oracle elsewhere (test_gpu_parity.py, test_gpu_dll_exact.py,
test_gpu_bank_lifecycle.py); this file only witnesses the path.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

import track_plan_model as model
from gypsum_amd import _lib
from gypsum_amd._lib import CHAN_INIT, SYNTH_SAT, GypsumHipError

pytestmark = pytest.mark.gpu

FS_2, FS_8 = 2_046_000, 8_184_000
N_MS = 300
SWITCH_DEFAULTS = {"no_pipe": 0, "no_spec": 0, "spec_redo": 1, "spec_sub_ms": 0, "track_chunk_ms": 250, "no_exact_shared": 0}


class _Rig:
    """One stream x 300 ms of 25 synthetic satellites in device memory, made once per rate."""

    def __init__(self, eng, fs):
        self.eng, self.fs, self.n = eng, fs, fs // 1000
        rng = np.random.default_rng(7300 + self.n)
        self.scene = np.zeros((1, 25), dtype=SYNTH_SAT)
        self.scene[0]["sat_id"] = np.arange(1, 26)
        self.scene[0]["code_phase"] = rng.integers(0, self.n, 25)
        self.scene[0]["doppler_hz"] = rng.uniform(-4500, 4500, 25)
        self.scene[0]["carrier_phase"] = rng.uniform(0, 2 * np.pi, 25)
        self.scene[0]["amplitude"] = 0.005 if self.n >= 8184 else 0.010
        self.scene[0]["nav_bit_offset_ms"] = rng.integers(0, 20, 25)
        self.stride = N_MS * self.n
        self.iq = eng.alloc(self.stride * 8)
        eng.synth_iq(self.iq, 1, self.stride, N_MS, self.scene, 0.03 if self.n >= 8184 else 0.05, 73)
        t = np.array([round(ms * self.n / fs, 6) for ms in range(N_MS)], dtype=np.float64)
        self.t_dev = eng.alloc(t.nbytes).upload(t)
        self.n_cus = int(re.search(r"(\d+) CUs\)$", eng.device_name()).group(1))      # the count the library plans with

    def inits(self, n_chan):
        s = self.scene[0]
        return np.array([(0, int(s["sat_id"][c]), float(round(float(s["doppler_hz"][c]))), float(s["carrier_phase"][c]) + 0.1, int(s["code_phase"][c]), 0)
                         for c in range(n_chan)], dtype=CHAN_INIT)

    def free(self):
        self.iq.free()
        self.t_dev.free()


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


def _track(rig, n_chan, n_ms, switches, keep=0):
    """One block on a fresh bank under `switches`; (plan of the model, last_track_flow, first two of spec_redo_read, last_exact_path,
    launches of the timed call)."""
    eng = rig.eng
    sw = dict(SWITCH_DEFAULTS, **switches)
    plan = model.track_plan(rig.n // 1023, rig.n, rig.n_cus, n_chan, n_ms, keep_profiles=int(keep > 0), kappa=20.0, **sw)
    bank = eng.create_bank(rig.inits(n_chan))
    timing = np.zeros(4, dtype=np.float32)
    redo = np.zeros(4, dtype=np.int32)
    try:
        for name, value in sw.items():
            eng.debug_set(name, value)
        if keep:
            bank.keep_profiles(keep)
        eng._check(eng.lib.gyp_debug_track_timing(eng.ctx, 1, None))
        bank.track_block_dev(rig.iq.ptr.value, rig.stride, n_ms, rig.t_dev.ptr.value)
        eng.sync()
        eng._check(eng.lib.gyp_debug_track_timing(eng.ctx, 1, _lib.ptr(timing)))
        eng._check(eng.lib.gyp_debug_spec_redo_read(bank.handle, _lib.ptr(redo)))
        return plan, int(eng.debug_get("last_track_flow")), redo[:2].tolist(), int(eng.debug_get("last_exact_path")), int(timing[3])
    finally:
        eng._check(eng.lib.gyp_debug_track_timing(eng.ctx, 0, None))
        for name, value in SWITCH_DEFAULTS.items():
            eng.debug_set(name, value)
        bank.close()


# id -> (rate, channels, block length, switches, kept profile rows, what the plan must be: the figures of the case as they are written down)
CASES = {
    "defaults": (FS_2, 2, 300, {}, 0, {"flow": 3, "n": 4, "rounds": 8, "starts": [0, 75, 150, 225, 300]}),
    "spec_redo_0": (FS_2, 2, 300, {"spec_redo": 0}, 0, {"flow": 2, "n": 4}),
    "block_of_200_ms": (FS_2, 2, 200, {}, 0, {"flow": 2, "n": 1}),
    "25_channels": (FS_2, 25, 300, {}, 0, {"flow": 2, "n": 4}),
    "no_spec": (FS_2, 2, 300, {"no_spec": 1}, 0, {"flow": 1, "launches": 2, "exact_path": 1}),
    "no_spec_whole_blocks": (FS_2, 2, 300, {"no_spec": 1, "track_chunk_ms": 0}, 0, {"flow": 1, "launches": 1, "exact_path": 1}),
    "keep_profiles": (FS_2, 2, 300, {}, 4, {"flow": 1, "launches": 2, "exact_path": 1}),
    "8184_no_spec": (FS_8, 2, 300, {"no_spec": 1}, 0, {"flow": 1, "launches": 2, "exact_path": 2}),
    "8184_no_spec_no_exact_shared": (FS_8, 2, 300, {"no_spec": 1, "no_exact_shared": 1}, 0, {"flow": 1, "launches": 2, "exact_path": 1}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_what_ran_is_what_the_plan_said(rigs, case):
    fs, n_chan, n_ms, switches, keep, written = CASES[case]
    plan, flow, redo, exact_path, launches = _track(rigs(fs), n_chan, n_ms, switches, keep)
    for field, value in written.items():
        assert plan[field] == value, (field, plan)
    assert flow == plan["flow"]
    if plan["flow"] == 1:
        assert exact_path == plan["exact_path"] and launches == plan["launches"]
        assert redo == [0, 0]                      # a fresh bank that has not tracked a block on the speculative path
    else:
        assert redo == [plan["n"], plan["rounds"] if plan["flow"] == 3 else plan["n"]]
        assert launches == 0                       # (the speculative path records no per-kernel times)


def test_speculative_blocks_leave_last_exact_path_alone(rigs):
    """ "last_exact_path" belongs to the last PLAIN throughput call: neither a speculative block nor its re-run of failed channels (which
    takes the per-channel kernel) touches it."""
    rig = rigs(FS_8)
    assert _track(rig, 2, 300, {"no_spec": 1})[3] == 2
    plan, flow, redo, exact_path, _ = _track(rig, 2, 300, {})
    assert (plan["flow"], flow, redo) == (3, 3, [plan["n"], plan["rounds"]]) and exact_path == 2
    plan, flow, _, exact_path, _ = _track(rig, 2, 300, {"spec_redo": 0})
    assert (plan["flow"], flow) == (2, 2) and exact_path == 2
    assert _track(rig, 2, 300, {"no_spec": 1, "no_exact_shared": 1})[3] == 1
    assert _track(rig, 2, 300, {})[3] == 1


def test_last_track_flow_is_read_only(rigs):
    eng = rigs(FS_2).eng
    before = eng.debug_get("last_track_flow")
    with pytest.raises(GypsumHipError):
        eng.debug_set("last_track_flow", 1)
    assert eng.debug_get("last_track_flow") == before
