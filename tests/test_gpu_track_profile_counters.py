"""The 16 cycle counters of gyp_debug_track_profile, as include/gypsum_hip.h documents them, for both forms of track_block_kernel.

A one-channel bank on a clean synthetic scene is tracked through 40 ms in one call with the counters armed; lane 0 of the wavefront
"prof_wave" names, in workgroup 0, keeps them.  Cycle counts are only asked to be positive or zero; the two counts of milliseconds
([4] all, [5] those on the transform path of the speculative form) are compared with the call's records.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from gypsum_amd import _lib, synth
from oracle import gypsum_oracle as orc

N_MS = 40


@functools.lru_cache(maxsize=None)
def _inputs(k):
    fs, n = 1_023_000 * k, 1023 * k
    scene = synth.random_scene(fs, N_MS, 1, 770000 + k, max_code_phase=(2046 if n > 2046 else None))
    iq = synth.render(scene)
    iq.setflags(write=False)
    sat = scene.sats[0]
    inits = np.zeros(1, dtype=_lib.CHAN_INIT)
    inits[0] = (0, sat.sat_id, float(round(sat.doppler_hz)), float(sat.carrier_phase), sat.code_phase, 0)
    t0 = np.array([orc.chunk_times(ms * n, n, fs)[0] for ms in range(N_MS)])
    return iq, inits, t0


@pytest.fixture(scope="module")
def engine():
    """GypsumEngine per (rate, speculative tracker allowed)."""
    from gypsum_amd.engine import GypsumEngine

    cache = {}

    def make(k, spec):
        if (k, spec) not in cache:
            eng = GypsumEngine(0)
            eng.set_stream_format(1_023_000 * k, 1023 * k)
            eng.debug_set("no_spec", 0 if spec else 1)
            cache[(k, spec)] = eng
        return cache[(k, spec)]

    yield make
    for eng in cache.values():
        eng.close()


def _profile(eng, enable, out=None):
    eng._check(eng.lib.gyp_debug_track_profile(eng.ctx, int(enable), out.ctypes.data if out is not None else None))


def _tracked(eng, k, prof_wave):
    """One armed call over the 40 ms from a fresh bank: (counters, records, last_track_flow); disarmed again on return."""
    iq, inits, t0 = _inputs(k)
    tp = np.full(16, -1, dtype=np.int64)
    eng.debug_set("prof_wave", prof_wave)
    _profile(eng, 1)
    try:
        bank = eng.create_bank(inits)
        rec = bank.track_block(iq, 1, N_MS, t0)
        flow = int(eng.debug_get("last_track_flow"))
        _profile(eng, 1, tp)
        bank.close()
    finally:
        _profile(eng, 0)
        eng.debug_set("prof_wave", 0)
    print(f"K={k} prof_wave={prof_wave} flow={flow} counters={tp.tolist()}")
    return tp, rec, flow


@pytest.mark.gpu
def test_throughput_form_wavefront_0(engine):
    """K = 8: 40 milliseconds, every phase took cycles, no transform-path count, and wavefront 0 -- the one that runs the Costas update --
    has the leave-fetch and Costas cycles in slots 6 and 8."""
    tp, rec, flow = _tracked(engine(8, False), 8, 0)
    assert flow == 1 and np.all(rec["status"] == 0)
    assert tp[4] == N_MS and tp[5] == 0
    assert np.all(tp[0:4] > 0), tp
    assert tp[6] > 0 and tp[8] > 0, tp


@pytest.mark.gpu
def test_throughput_form_another_wavefront(engine):
    """K = 8, wavefront 1: the same phases, but slots 6 and 8 stay 0 -- only wavefront 0 runs the Costas update."""
    tp, rec, flow = _tracked(engine(8, False), 8, 1)
    assert flow == 1
    assert tp[4] == N_MS and tp[5] == 0
    assert np.all(tp[0:4] > 0), tp
    assert tp[6] == 0 and tp[8] == 0, tp


@pytest.mark.gpu
def test_throughput_form_clamps_the_wavefront(engine):
    """K = 2 has two wavefronts: "prof_wave" 7 is clamped to the last one by the launcher, so the counters are this call's."""
    tp, rec, flow = _tracked(engine(2, False), 2, 7)
    assert flow == 1
    assert tp[4] == N_MS, tp


@pytest.mark.gpu
def test_speculative_form(engine):
    """K = 8 on the speculative tracker: [4] counts the milliseconds the channel was tracked through, [5] those of them that took the
    transform path (path_info bit 0 clear), and the stamp-to-stamp slots 6..15 hold cycles."""
    tp, rec, flow = _tracked(engine(8, True), 8, 0)
    assert flow in (2, 3)
    tracked = rec["status"][0] == 0
    assert tp[4] == np.count_nonzero(tracked), (tp, rec["status"][0])
    assert tp[5] == np.count_nonzero(tracked & ((rec["path_info"][0] & 1) == 0)), (tp, rec["path_info"][0])
    assert np.sum(tp[6:16]) > 0, tp


@pytest.mark.gpu
def test_disarmed_leaves_the_buffer_alone(engine):
    eng = engine(8, False)
    tp, _, _ = _tracked(eng, 8, 0)          # (disarmed on return)
    before = tp.copy()
    iq, inits, t0 = _inputs(8)
    bank = eng.create_bank(inits)
    bank.track_block(iq, 1, N_MS, t0)
    _profile(eng, 0, tp)
    bank.close()
    assert np.array_equal(tp, before)
