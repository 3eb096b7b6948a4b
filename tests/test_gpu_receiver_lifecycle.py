"""BatchedGpsReceiver across a loss, a re-queue, a second scan and a slot revival, against the float64 receiver model.

Scenes R1, R2, R3 (tests/lifecycle_scenes.py): satellite X leaves, the circularity watchdog drops it, it goes back on the search list,
a later scan acquires it again and its bank slot starts a second life whose first millisecond is a watchdog look at a single peak.
R1 runs with the reference's constants (scan every 10 s, watchdog every 6 s, a search list that never empties: the re-scan waits for the
10-s mark); R2 and R3 with a scan period of 1 s and a watchdog period of 0.6 s and a search list that empties (the scan timestamp goes
stale: the drop is followed by a scan at the very next millisecond).  The reference is tests/receiver_model.py, float64 throughout;
the conditions a scene must show there are asserted first (lifecycle_scenes.scene_conditions), the device is compared afterwards.

Smallest margins the model recorded with the chosen seeds (relative lock margin, |circularity - 0.2|, |circularity - 0.93|,
|strength - 3|):   R1 1.08e-4, 0.168, 0.069, 0.38;   R2 1.02e-4, 0.119, 0.047, 0.75;   R3 7.7e-4, 0.019, 0.045, 0.47.
"""
from __future__ import annotations

import dataclasses
import time

import numpy as np
import pytest

import lifecycle_scenes as ls
import receiver_model as rm
from gypsum_amd import receiver as receiver_module
from gypsum_amd import tracker as tracker_module
from gypsum_amd.antenna_sample_provider import AntennaSampleProviderBackedByArray, NoMoreSamplesError
from gypsum_amd.engine import default_engine
from gypsum_amd.gps_ca_prn_codes import GpsSatelliteId
from gypsum_amd.navigation_bit_intergrator import _BIT_VALUES
from gypsum_amd.receiver import BatchedGpsReceiver, GpsReceiver
from oracle import gypsum_oracle as orc

pytestmark = pytest.mark.gpu

_cache = {}


def _scene(spec):
    """(iq, search list, X, the model's finished run) of a scene, once per session; the model's lives run in worker processes."""
    if spec.name not in _cache:
        iq, search, x = spec.build()
        t = time.perf_counter()
        with rm.shared_samples(iq, len(search)) as (path, pool):
            model = ls.run_model(spec, path, search, pool)
        print(f"[{spec.name}] model: {time.perf_counter() - t:.1f} s, {model.channel_ms()} channel-ms, scans at {[s.step for s in model.scans]}, "
              f"margins {({k: float(f'{v:.3e}') for k, v in model.margins().items()})}")
        assert ls.scene_conditions(model, x) == [], spec.name
        _cache[spec.name] = (iq, search, x, model)
    return _cache[spec.name]


class _Run:
    """One BatchedGpsReceiver run over a scene with everything the comparison needs recorded on the way."""

    def __init__(self, spec, iq, search, block_ms, chunks):
        fs, n = spec.fs, spec.fs // 1000
        self.n = n
        eng = default_engine(fs, n)
        old_params, old_scan = eng.get_params(), receiver_module.ACQUISITION_SCAN_FREQUENCY
        self.blocks, self.scans, self.sets, self.states, self.rows, self.events = [], [], [], [], {}, {}
        try:
            eng.set_params(watchdog_period_s=spec.watchdog_period_s)
            receiver_module.ACQUISITION_SCAN_FREQUENCY = spec.scan_period_s
            rx = BatchedGpsReceiver(AntennaSampleProviderBackedByArray(iq, fs), only_acquire_satellite_ids=[GpsSatelliteId(s) for s in search],
                                    block_ms=block_ms)
            self.rx = rx
            bank, detector, provider = rx._bank, rx.satellite_detector, rx.antenna_samples_provider
            track, set_channel, detect, get_block = bank.track_block, bank.set_channel, detector.detect_satellites_in_antenna_data, provider.get_block

            def rec_track(iq_, n_streams, n_ms, t0, *a, **k):
                rec = track(iq_, n_streams, n_ms, t0, *a, **k)
                self.blocks.append((rx.steps_done, n_ms, [s.id for s in rx.tracked_satellite_ids_to_tracking_params]))
                for sid in rx.tracked_satellite_ids_to_tracking_params:
                    self.rows.setdefault(sid.id, []).append((rx.steps_done, rec[sid.id - 1].copy()))
                return rec

            def rec_set(index, init):
                self.sets.append((rx.steps_done, index, tuple(init)))
                return set_channel(index, init)

            def rec_detect(ids, samples, attrs):
                found = detect(ids, samples, attrs)
                self.scans.append((rx.steps_done, [s.id for s in ids], list(found)))
                return found

            def rec_get_block(length):            # the top of every turn of run()'s loop: the lists as the previous turn left them
                self._snapshot()
                return get_block(length)

            bank.track_block, bank.set_channel, detector.detect_satellites_in_antenna_data, provider.get_block = rec_track, rec_set, rec_detect, rec_get_block
            k = 0
            while True:
                try:
                    out = rx.run(chunks[k % len(chunks)])
                except NoMoreSamplesError:
                    break
                k += 1
                for sid, ev in out.items():
                    self.events.setdefault(sid.id, []).extend(ev)
            self._snapshot()
        finally:
            receiver_module.ACQUISITION_SCAN_FREQUENCY = old_scan
            eng.set_params(**old_params)

    def _snapshot(self):
        state = ([s.id for s in self.rx.tracked_satellite_ids_to_tracking_params], [s.id for s in self.rx.satellite_ids_eligible_for_acquisition])
        if not self.states or self.states[-1] != state:
            self.states.append(state)

    def life_rows(self, sat, first, end):
        """The bank's records of satellite `sat` for steps [first, end), out of the blocks that were tracked while it was tracked."""
        parts = [(s, r) for s, r in self.rows.get(sat, []) if s + len(r) > first and s < end]
        assert parts and parts[0][0] == first, (sat, first, [p[0] for p in parts][:3])
        got = np.concatenate([r for _, r in parts])
        assert [s for s, _ in parts] == list(np.cumsum([first] + [len(r) for _, r in parts[:-1]]))      # contiguous
        return got[:end - first]


def _compare(spec, model, x, run):
    n, fs = spec.fs // 1000, spec.fs
    rx = run.rx
    assert rx.steps_done == spec.n_ms == model.steps_done
    # scans: the same steps, the same list handed to each, the same results
    worst_phase = 0.0
    assert [(s, ids) for s, ids, _ in run.scans] == [(sc.step, sc.sat_ids) for sc in model.scans]
    for (step, _, found), sc in zip(run.scans, model.scans):
        assert [r.satellite_id.id for r in found] == sc.acquired, step
        for r in found:
            want = next(l.acquisition for l in model.lives[r.satellite_id.id] if l.acquired_at == step)
            assert (r.doppler_shift, r.prn_phase_shift) == (want.doppler_shift, want.prn_phase_shift), (step, r.satellite_id)
            err = float(abs(np.angle(np.exp(1j * (r.carrier_wave_phase_shift - want.carrier_wave_phase_shift)))))
            worst_phase = max(worst_phase, err)
            assert err < 1e-6, (step, r.satellite_id, err)                      # carrier phase to a microradian
    print(f"[{spec.name}] largest carrier-phase difference of an acquisition: {worst_phase:.3e} rad")
    # every acquisition revives the satellite's own slot, at the scan's step
    assert [(s, i) for s, i, _ in run.sets] == [(sc.step, sv - 1) for sc in model.scans for sv in sc.acquired]
    # tracked set and eligible list, in order, after every change and at the end
    assert run.states == [([], list(model.scans[0].sat_ids))] + [(t, e) for _, t, e in model.changes]
    assert [s.id for s in rx.tracked_satellite_ids_to_tracking_params] == list(model.tracked) and \
           [s.id for s in rx.satellite_ids_eligible_for_acquisition] == model.eligible
    # life by life
    channel_ms = 0
    for sat, lives in model.lives.items():
        emitted = rx.emitted_pseudosymbols[GpsSatelliteId(sat)]
        assert len(emitted) == sum(len(l.records) for l in lives), sat
        at = 0
        for life in lives:
            rows = life.records
            end = life.acquired_at + len(rows) + (1 if life.lost_at is not None else 0)
            g = run.life_rows(sat, life.acquired_at, end)
            if life.lost_at is not None:                                   # the same loss step: status 1 there, 0 before
                assert life.lost_at == end - 1 and g[-1]["status"] == 1, (sat, life.lost_at)
                g = g[:-1]
            assert not g["status"].any(), sat
            for name, want in (("pseudosymbol", [r.pseudosymbol for r in rows]), ("code_phase", [r.code_phase_after for r in rows]),
                               ("locked", [int(r.locked) for r in rows]), ("nudged", [int(r.nudged) for r in rows])):
                bad = np.flatnonzero(g[name].astype(np.int64) != np.array(want, dtype=np.int64))
                assert bad.size == 0, (sat, life.acquired_at, name, "first at millisecond", int(bad[0]), bad.size)
            assert np.abs(g["doppler_hz"] - np.array([r.doppler_after for r in rows])).max() < 1e-3, (sat, life.acquired_at)
            mine = emitted[at:at + len(rows)]
            at += len(rows)
            assert [e.pseudosymbol.as_val() for e in mine] == [r.pseudosymbol for r in rows]
            assert [e.start_of_pseudosymbol for e in mine] == [r.start_of_pseudosymbol for r in rows], (sat, life.acquired_at)
            channel_ms += len(rows)
        # navigation bits: time stamps and values; a second life's integrator starts empty, so its first bit begins in that life
        want = [(a, b, _BIT_VALUES[v]) for life in lives for a, b, v in life.bit_events]
        got = [(e.receiver_timestamp, e.trailing_edge_receiver_timestamp, e.bit_value) for e in run.events.get(sat, [])]
        assert got == want, sat
        for life in lives[1:]:
            assert life.bit_events and life.bit_events[0][0] >= orc.chunk_times(life.acquired_at * n, n, fs)[0]
    assert len(model.lives[x]) == 2 and all(len(l.bit_events) > 5 for l in model.lives[x])
    # the block cutting, seen at the bank's track_block
    looks = {lk.step for _, lk in model.looks()}
    ends = {s + k - 1 for s, k, _ in run.blocks}
    assert looks <= ends, sorted(looks - ends)                             # a block ends at every step at which a watchdog looks
    scan_steps = {sc.step for sc in model.scans}
    for s, k, _ in run.blocks:                                             # no block spans a scan step: one may only START there
        assert not any(s < step < s + k for step in scan_steps), (s, k)
    second = model.lives[x][1]
    assert orc.chunk_times(second.acquired_at * n, n, fs)[0] >= spec.watchdog_period_s
    assert [k for s, k, _ in run.blocks if s == second.acquired_at] == [1]      # the revived life's first block: its look, alone
    return channel_ms


RUNS = [(1, (1000,)), (128, (7, 100, 250, 1000)), (250, (333, 64, 1, 1000)), (1000, (3500,))]


@pytest.mark.parametrize("block_ms,chunks", RUNS)
@pytest.mark.parametrize("spec", [ls.R2, ls.R3], ids=lambda s: s.name)
def test_short_periods_any_block_length_any_run_chunks(spec, block_ms, chunks):
    iq, search, x, model = _scene(spec)
    t = time.perf_counter()
    channel_ms = _compare(spec, model, x, _Run(spec, iq, search, block_ms, chunks))
    print(f"[{spec.name}] block_ms {block_ms}, run() chunks {chunks}: {channel_ms} channel-ms equal the model's, {time.perf_counter() - t:.1f} s")


def test_reference_constants_the_rescan_waits_for_the_ten_second_mark():
    spec = ls.R1
    iq, search, x, model = _scene(spec)
    first, second = model.lives[x]
    assert [sc.step for sc in model.scans] == [9, 10009] and model.scans[1].sat_ids == [s for s in search if s not in model.scans[0].acquired] + [x]
    assert first.lost_at == 6000 and second.acquired_at == 10009
    channel_ms = _compare(spec, model, x, _Run(spec, iq, search, 250, (4000, 1, 999, 4000, 10000)))
    print(f"[R1] {channel_ms} channel-ms equal the model's")


def test_a_block_longer_than_the_scan_period_is_cut_at_every_scan():
    """R1's first 900 ms with a scan every 0.2 s and block_ms = 1000.  Two satellites of the search list are not in the scene, so the
    list never empties and a scan runs every period; no watchdog looks before 6 s, so nothing but the scans cuts a block.  A block
    that begins with a scan must end before the next scan, which that very scan has just scheduled."""
    spec = dataclasses.replace(ls.R1, name="R1-scans", n_ms=900, scan_period_s=0.2)
    iq, search, x = spec.build()
    with rm.shared_samples(iq, len(search)) as (path, pool):
        model = ls.run_model(spec, path, search, pool)
    steps = [sc.step for sc in model.scans]
    assert steps[0] == 9 and len(steps) == 5 and all(b - a in (200, 201) for a, b in zip(steps, steps[1:])) and all(not sc.acquired for sc in model.scans[1:])
    assert model.margins()["strength"] >= ls.MIN_STRENGTH_MARGIN and not model.looks()
    run = _Run(spec, iq, search, 1000, (900,))
    assert run.rx.steps_done == spec.n_ms
    assert [(s, ids, [r.satellite_id.id for r in found]) for s, ids, found in run.scans] == [(sc.step, sc.sat_ids, sc.acquired) for sc in model.scans]
    assert [(s, k) for s, k, _ in run.blocks] == [(a, b - a) for a, b in zip(steps, steps[1:] + [spec.n_ms])]
    for sat, (life,) in model.lives.items():
        g = run.life_rows(sat, life.acquired_at, spec.n_ms)
        assert not g["status"].any()
        assert [int(v) for v in g["pseudosymbol"]] == [r.pseudosymbol for r in life.records], sat
        assert [int(v) for v in g["code_phase"]] == [r.code_phase_after for r in life.records], sat
        assert np.abs(g["doppler_hz"] - np.array([r.doppler_after for r in life.records])).max() < 1e-3, sat


def test_the_per_millisecond_receiver_is_a_third_witness_on_r2():
    """GpsReceiver.step() once per millisecond (host loop filters around gyp_track_step, its own watchdog clock per tracker object,
    the reference's scan rule verbatim) over R2: the same lives as the model's."""
    spec = ls.R2
    iq, search, x, model = _scene(spec)
    fs, n = spec.fs, spec.fs // 1000
    events, log = {}, []
    old = (receiver_module.ACQUISITION_SCAN_FREQUENCY, tracker_module._WATCHDOG_PERIOD_SECONDS)
    receiver_module.ACQUISITION_SCAN_FREQUENCY, tracker_module._WATCHDOG_PERIOD_SECONDS = spec.scan_period_s, spec.watchdog_period_s
    try:
        rx = GpsReceiver(AntennaSampleProviderBackedByArray(iq, fs), only_acquire_satellite_ids=[GpsSatelliteId(s) for s in search],
                         on_events=lambda sid, ev: events.setdefault(sid.id, []).extend(ev))
        pipes = {}
        for step in range(spec.n_ms):
            rx.step()
            now = {sid.id: p for sid, p in rx.tracked_satellite_ids_to_processing_pipelines.items()}
            for sat, p in now.items():
                if pipes.get(sat) is not p:
                    log.append(("acquired", step, sat, p))
            for sat, p in pipes.items():
                if now.get(sat) is not p:
                    log.append(("lost", step, sat, p))
            pipes = now
        with pytest.raises(NoMoreSamplesError):
            rx.step()
    finally:
        receiver_module.ACQUISITION_SCAN_FREQUENCY, tracker_module._WATCHDOG_PERIOD_SECONDS = old
    assert [s.id for s in rx.tracked_satellite_ids_to_processing_pipelines] == list(model.tracked)
    assert [s.id for s in rx.satellite_ids_eligible_for_acquisition] == model.eligible
    want_log = sorted([("acquired", l.acquired_at, sv) for sv, lives in model.lives.items() for l in lives] +
                      [("lost", l.lost_at, sv) for sv, lives in model.lives.items() for l in lives if l.lost_at is not None], key=lambda e: (e[1], e[0], e[2]))
    assert sorted([e[:3] for e in log], key=lambda e: (e[1], e[0], e[2])) == want_log
    for kind, step, sat, pipe in log:
        if kind != "acquired":
            continue
        life = next(l for l in model.lives[sat] if l.acquired_at == step)
        got = pipe.emitted_pseudosymbols
        assert [e.pseudosymbol.as_val() for e in got] == [r.pseudosymbol for r in life.records], (sat, step)
        assert [e.start_of_pseudosymbol for e in got] == [r.start_of_pseudosymbol for r in life.records], (sat, step)
        dop = np.array(pipe.tracker.tracking_params.doppler_shifts[:len(life.records)])
        assert np.abs(dop - np.array([r.doppler_after for r in life.records])).max() < 1e-3, (sat, step)
    for sat, lives in model.lives.items():
        want = [(a, b, _BIT_VALUES[v]) for life in lives for a, b, v in life.bit_events]
        assert [(e.receiver_timestamp, e.trailing_edge_receiver_timestamp, e.bit_value) for e in events.get(sat, [])] == want, sat
