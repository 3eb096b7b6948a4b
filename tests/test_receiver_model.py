"""Host: the leave-and-return scene helper and the float64 receiver model (tests/lifecycle_scenes.py, tests/receiver_model.py).

The model is the reference of tests/test_gpu_receiver_lifecycle.py; here it runs scene R2 alone (short periods: scan every 1 s,
watchdog every 0.6 s) and must show, without any device, the schedule the scene was built for: X dropped by the watchdog, the stale
scan timestamp of an emptied search list answered by a scan at the very next millisecond, scans repeated every period while X is
absent, X acquired again, and a second life whose first millisecond is a watchdog look at a single peak.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

import lifecycle_scenes as ls
import receiver_model as rm
from gypsum_amd import synth
from oracle import gypsum_oracle as orc


def test_all_ones_masks_give_the_plain_render():
    """The parts are rounded to float32 one by one (synth.render stores complex64): per component the sum of k parts and the noise
    differs from the direct render by at most 2^-24 (sum of the parts' magnitudes) for those roundings, plus 2^-24 |x| for each of the
    two final casts."""
    scene = synth.lock_regime_scene(2_046_000, 60, 7)
    want = synth.render(scene)
    ones = {s.sat_id: np.ones(scene.n_ms, dtype=np.int8) for s in scene.sats}
    for presence in ({}, ones):
        got = ls.render_with_presence(scene, presence)
        assert got.dtype == np.complex64 and got.shape == want.shape
        parts = sum(s.amplitude for s in scene.sats) + np.abs(synth.render(dataclasses.replace(scene, sats=[])))
        bound = 2.0 ** -24 * (parts + 2 * np.abs(want)) * 1.01
        assert np.all(np.abs(got.real - want.real) <= bound) and np.all(np.abs(got.imag - want.imag) <= bound)


def test_a_masked_satellite_is_gone_for_exactly_its_milliseconds():
    scene = synth.lock_regime_scene(2_046_000, 40, 7)
    n = scene.samples_per_ms
    x = scene.sats[0]
    mask = np.ones(scene.n_ms, dtype=np.int8)
    mask[10:25] = 0
    got = ls.render_with_presence(scene, {x.sat_id: mask})
    full = ls.render_with_presence(scene, {})
    without = ls.render_with_presence(dataclasses.replace(scene, sats=scene.sats[1:]), {})
    assert np.array_equal(got[:10 * n], full[:10 * n]) and np.array_equal(got[25 * n:], full[25 * n:])
    assert np.array_equal(got[10 * n:25 * n], without[10 * n:25 * n])
    assert not np.array_equal(got[10 * n:25 * n], full[10 * n:25 * n])
    with pytest.raises(ValueError):
        ls.render_with_presence(scene, {x.sat_id: mask[:-1]})
    with pytest.raises(ValueError):
        ls.render_with_presence(scene, {x.sat_id: mask * 2})


@pytest.fixture(scope="module")
def r2():
    iq, search, x = ls.R2.build()
    with rm.shared_samples(iq, len(search)) as (path, pool):
        model = ls.run_model(ls.R2, path, search, pool)
    return iq, search, x, model


def test_r2_meets_every_scene_condition(r2):
    iq, search, x, model = r2
    print(f"R2: margins {model.margins()}, {model.channel_ms()} channel-ms, scans at {[sc.step for sc in model.scans]}")
    assert ls.scene_conditions(model, x) == []
    assert model.steps_done == ls.R2.n_ms
    assert rm.ACQUISITION_SCAN_FREQUENCY == 10 and orc.WATCHDOG_PERIOD_S == 6       # the patched periods were put back


def test_r2_scan_schedule_follows_the_stale_timestamp_rule(r2):
    """receiver.py:148-163: the first scan runs when ten chunks are buffered and empties the search list; the timestamp is then not
    refreshed, so the drop of X is followed by a scan at the very next millisecond; that one fails (X is absent) and refreshes the
    timestamp, and scans repeat once per period until X is back."""
    iq, search, x, model = r2
    first, second = model.lives[x][:2]
    steps = [sc.step for sc in model.scans]
    assert steps[0] == 9 and model.scans[0].sat_ids == search and model.scans[0].acquired == search
    assert steps[1] == first.lost_at + 1 and model.scans[1].sat_ids == [x] and model.scans[1].acquired == []
    assert first.lost_at < ls.R2.absent_ms[1] <= second.acquired_at
    n, fs = ls.R2.fs // 1000, ls.R2.fs
    for a, b in zip(model.scans[1:], model.scans[2:]):          # the next scan: the first millisecond whose end is a period later
        assert b.sat_ids == [x]
        assert orc.chunk_times(b.step * n, n, fs)[1] - orc.chunk_times(a.step * n, n, fs)[1] >= ls.R2.scan_period_s
        assert orc.chunk_times((b.step - 1) * n, n, fs)[1] - orc.chunk_times(a.step * n, n, fs)[1] < ls.R2.scan_period_s
    assert model.scans[-1].step == second.acquired_at and model.scans[-1].acquired == [x]
    assert len(model.scans) >= 3
    # tracked set and eligible list after every change: the scan, the drop, the re-acquisition (X moves to the END of the dict)
    others = [sv for sv in search if sv != x]
    assert model.changes == [(9, search, []), (first.lost_at, others, [x]), (second.acquired_at, others + [x], [])]


def test_r2_lives_are_fresh_trackers_and_integrators(r2):
    """Each life equals a new orc.Tracker / orc.BitIntegrator started from its acquisition at its step -- the watchdog clock at 0, so
    the second life looks in its first millisecond -- and a scan is orc.detect_satellites on the ten newest chunks."""
    iq, search, x, model = r2
    n, fs = ls.R2.fs // 1000, ls.R2.fs
    chips = orc.generate_ca_codes()
    second = model.lives[x][1]
    step = second.acquired_at
    found = orc.detect_satellites([x], iq[(step - 9) * n:(step + 1) * n], fs, n, {x: orc.prn_as_complex(chips[x - 1], n)})
    assert [dataclasses.astuple(r) for r in found] == [dataclasses.astuple(second.acquisition)]
    old = orc.WATCHDOG_PERIOD_S
    orc.WATCHDOG_PERIOD_S = ls.R2.watchdog_period_s
    try:
        a = second.acquisition
        trk = orc.Tracker(orc.TrackingState(a.doppler_shift, a.carrier_wave_phase_shift, a.prn_phase_shift),
                          orc.prn_as_complex(chips[x - 1], n), fs, n)
        bits, events = orc.BitIntegrator(), []
        for k, want in enumerate(second.records[:300]):
            t0, t1 = orc.chunk_times((step + k) * n, n, fs)
            got = trk.process_samples(iq[(step + k) * n:(step + k + 1) * n], t0, t1)
            assert (got.pseudosymbol, got.code_phase_after, got.locked, got.doppler_after) == \
                   (want.pseudosymbol, want.code_phase_after, want.locked, want.doppler_after), k
            events += bits.process(t0, got.start_of_pseudosymbol, got.end_of_pseudosymbol, got.pseudosymbol)[1]
            if k == 0:
                assert trk._last_circularity_check == t0 >= ls.R2.watchdog_period_s
    finally:
        orc.WATCHDOG_PERIOD_S = old
    assert events and events == second.bit_events[:len(events)]
    assert not any(r.locked for r in second.records[:249])          # a fresh lock window: 250 errors before it can lock
    assert second.looks[0].n_peaks == 1 and second.looks[1].n_peaks == 2 + second.looks[1].step - step - 1
