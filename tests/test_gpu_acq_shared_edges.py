"""Shared forward transforms of the acquisition search at their edges, with a witness of the path taken.

test_gpu_acq_shared_fwd.py holds "switch off == switch on, byte for byte" at one shape.  That alone cannot tell a library that shares
from one that never does.  gyp_debug_get "last_acq_units" / "last_acq_shared_cells" / "last_acq_unshared_cells" say what the levels of
the last search did (units given a forward pass of their own, cells that read a unit's spectra, cells on the unshared list); here they
are held against the CPU model of the planner (acq_units_model.py) -- exactly, for single levels with every state on one centre and
for whole scans whose level winners come from the float64 oracle's trace -- and every byte comparison also asserts that the shared run
shared and the switched-off run did not.  Shapes: the spectra buffer's 1 GiB cap reached inside a stream (n_ms = 40), n_ms = 1, 2, 3
and 21, strided NaN-guarded layouts, odd satellite lists, scans split over helper contexts, one context reused across calls of
different sizes and rates, other launch geometries.

All inputs are synthetic.  "Byte-equal": the records with no_acq_shared_fwd = 0 equal those with 1, tobytes().  Oracle comparisons
use the bars of test_gpu_every_rate.py::test_full_sky_acquisition_at_every_rate: Doppler bin and code phase equal, strength within
1e-4."""
from __future__ import annotations

import multiprocessing as mp
import time

import numpy as np
import pytest

import survey_worker
from acq_units_model import (MAX_BINS, active_cells, expected_counts, expected_scan_counts, level_bins, max_units_for, plan_level,
                             scan_levels)
from gypsum_amd import _lib, synth
from gypsum_amd._lib import ACQ_RESULT, SYNTH_SAT
from gypsum_amd.engine import GypsumEngine
from test_gpu_every_rate import _dev_copy, _guarded
from test_gpu_params import ORACLE_NAME

pytestmark = pytest.mark.gpu
FS, N = 8_184_000, 8184
ALL_IDS = list(range(1, 33))
SAT_LISTS = {32: ALL_IDS, 31: list(range(1, 32)), 3: [31, 2, 17], 2: [7, 19], 1: [7]}
WITNESS = ("last_acq_units", "last_acq_shared_cells", "last_acq_unshared_cells")


# ------------------------------------------------------------------ helpers
def _engine(shared_off, fs=FS, n=N, params=None, **knobs):
    eng = GypsumEngine(0)
    eng.set_stream_format(fs, n)
    eng.debug_set("no_acq_shared_fwd", shared_off)
    for k, v in knobs.items():
        eng.debug_set(k, v)
    if params:
        eng.set_params(**params)
    return eng


def _witness(eng):
    """(units, shared cells, unshared cells) of the last search on the engine, helper contexts included."""
    return tuple(int(eng.debug_get(name)) for name in WITNESS)


def _witness_levels(eng, n_levels=3):
    """The same per level, for the first n_levels levels of the last search."""
    return [tuple(int(eng.debug_get(f"{name}_l{k}")) for name in WITNESS) for k in range(1, n_levels + 1)]


_SYNTH = {}


def _synth(n_streams, n_ms, seed=2026, fs=FS, n=N):
    """n_streams x n_ms of six planted satellites each (the last stream noise only), generated on the device, kept on the host."""
    key = (n_streams, n_ms, seed, fs)
    if key not in _SYNTH:
        rng = np.random.default_rng(seed)
        sats = np.zeros((n_streams, 6), dtype=SYNTH_SAT)
        for s in range(n_streams):
            sats[s]["sat_id"] = rng.choice(np.arange(1, 33), size=6, replace=False)
            sats[s]["code_phase"] = rng.integers(0, n, 6)
            sats[s]["doppler_hz"] = rng.uniform(-6500, 6500, 6)
            sats[s]["carrier_phase"] = rng.uniform(0, 2 * np.pi, 6)
            sats[s]["amplitude"] = 0.0 if (s == n_streams - 1 and n_streams > 1) else 40.0 / n
            sats[s]["nav_bit_offset_ms"] = rng.integers(0, 20, 6)
        gen = GypsumEngine(0)
        gen.set_stream_format(fs, n)
        iq = gen.alloc(n_streams * n_ms * n * 8)
        gen.synth_iq(iq, n_streams, n_ms * n, n_ms, sats, 6 * 40.0 / n, 4242 + seed)
        _SYNTH[key] = iq.download(np.complex64, n_streams * n_ms * n)
        iq.free()
        gen.close()
    return _SYNTH[key]


def _scan(eng, host, n_streams, n_ms, sat_ids, n=N):
    """gyp_acquire_dev of packed streams: (records, witness)."""
    buf = _dev_copy(eng, host[: n_streams * n_ms * n])
    out = eng.alloc(n_streams * len(sat_ids) * ACQ_RESULT.itemsize)
    eng.acquire_dev(buf.ptr.value, n_streams, n_ms * n, n_ms, sat_ids, out.ptr.value)
    w = _witness(eng)            # (waits for the scan, helper contexts included)
    eng.sync()
    rec = out.download(ACQ_RESULT, n_streams * len(sat_ids))
    buf.free()
    out.free()
    return rec, w


def _assert_off(w, where=""):
    assert w[0] == 0 and w[1] == 0, (where, w)


def _ab_scan(host, n_streams, n_ms, sat_ids, shares=True, **knobs):
    """A whole scan with the switch at 1 and at 0 on fresh engines: byte-equal, the switched-off run shared nothing and the shared
    run shared (or not, where it cannot); no cell lost or served twice.  Returns (records, witness of the shared run, of the other)."""
    off, on = _engine(1, **knobs), _engine(0, **knobs)
    try:
        want, w_off = _scan(off, host, n_streams, n_ms, sat_ids)
        got, w_on = _scan(on, host, n_streams, n_ms, sat_ids)
    finally:
        off.close()
        on.close()
    where = (n_streams, n_ms, len(sat_ids), knobs)
    assert got.tobytes() == want.tobytes(), (where, int(np.sum(got != want)))
    _assert_off(w_off, where)
    assert (w_on[0] > 0 and w_on[1] >= 2 * w_on[0]) if shares else (w_on[0] == 0 and w_on[1] == 0), (where, w_on)
    assert w_on[1] + w_on[2] == w_off[2], (where, w_on, w_off)
    return got, w_on, w_off


def _single_level_model(center, spread, n_streams, n_sats, n_ms):
    cells = plan_level(np.full((n_streams, n_sats), float(center)), spread, None)
    return expected_counts([cells], max_units_for(n_streams, n_sats, n_ms), n_sats)


def _oracle_traces(jobs):
    """jobs = [(fs, n_ms, seed, sat_id, changes)] through the float64 oracle in a pool: {(seed, sat_id): (doppler, code phase, strength,
    [level winners])}."""
    out = {}
    with mp.get_context("spawn").Pool(survey_worker.pool_size(len(jobs))) as pool:
        for seed, sv, dop, cp, strength, winners in pool.imap_unordered(survey_worker.run_acq_trace_one, jobs):
            out[(seed, sv)] = (dop, cp, strength, winners)
    return out


def _assert_oracle(rec, seeds, sat_ids, want, where):
    """The bars of test_full_sky_acquisition_at_every_rate."""
    for i, g in enumerate(rec):
        seed, sv = seeds[i // len(sat_ids)], sat_ids[i % len(sat_ids)]
        dop, cp, strength, _ = want[(seed, sv)]
        assert int(g["sat_id"]) == sv and int(g["stream"]) == i // len(sat_ids), (where, i)
        assert int(g["doppler_hz"]) == dop, (where, seed, sv, int(g["doppler_hz"]), dop)
        assert int(g["code_phase"]) == cp, (where, seed, sv, int(g["code_phase"]), cp)
        assert abs(float(g["strength"]) - strength) <= 1e-4 * strength, (where, seed, sv, float(g["strength"]), strength)


def _scene_iq(seeds, n_ms):
    return np.concatenate([synth.render(synth.random_scene(FS, n_ms, 6, seed, with_nav_bits=False, max_code_phase=2046)) for seed in seeds])


def _whole_scan_against_model(seeds, sat_ids, n_ms=10, params=None, label=""):
    """A scan of len(seeds) streams (one context: fewer than four streams are never split) with the switch at 0 and at 1: the records
    against the oracle, the three counters against the planner model fed with the oracle's level winners -- exactly."""
    t_start = time.time()
    params = params or {}
    changes = {ORACLE_NAME[k]: v for k, v in params.items() if k in ORACLE_NAME}
    want = _oracle_traces([(FS, n_ms, seed, sv, changes) for seed in seeds for sv in sat_ids])
    t_oracle = time.time() - t_start
    winners = [want[(seed, sv)][3] for seed in seeds for sv in sat_ids]
    kw = dict(initial_spread=params.get("acq_initial_spread_hz", 7000.0), min_spread=params.get("acq_min_spread_hz", 10.0),
              bins_per_spread=params.get("acq_bins_per_spread", 10.0), reuse=params.get("acq_reuse_level_records", 1.0) != 0.0)
    n_streams, n_sats = len(seeds), len(sat_ids)
    model_on = expected_scan_counts(winners, n_streams, n_sats, n_ms, True, **kw)
    model_off = expected_scan_counts(winners, n_streams, n_sats, n_ms, False, **kw)
    room = max_units_for(n_streams, n_sats, n_ms)
    per_level = [expected_counts([c], 10 ** 6, n_sats) for c in scan_levels(winners, n_streams, n_sats, **kw)[:3]]
    iq = _scene_iq(seeds, n_ms)
    off, on = _engine(1, params=params), _engine(0, params=params)
    try:
        rec_off, w_off = _scan(off, iq, n_streams, n_ms, sat_ids)
        rec_on, w_on = _scan(on, iq, n_streams, n_ms, sat_ids)
        dev_levels = _witness_levels(on)
    finally:
        off.close()
        on.close()
    print(f"[whole scan {label}: {n_streams} x {n_sats}, {params}] device {w_on} / switched off {w_off}; model {model_on} / {model_off}; "
          f"levels 1-3 (units, shared, unshared): device {dev_levels}, model without a cap {per_level}, room {room}; "
          f"oracle {t_oracle:.0f} s, all {time.time() - t_start:.0f} s")
    _assert_oracle(rec_on, seeds, sat_ids, want, label)
    assert rec_on.tobytes() == rec_off.tobytes(), label
    assert w_on == model_on, (label, w_on, model_on)
    assert w_off == model_off, (label, w_off, model_off)
    assert w_on[0] > 0
    assert dev_levels == [expected_counts([c], room, n_sats) for c in scan_levels(winners, n_streams, n_sats, **kw)[:3]]
    return per_level, room


# ------------------------------------------------------------------ 1. the planner kernel against the model, exact counts
LEVELS = [(0.0, 7000.0), (-2100.0, 3500.0), (1400.0, 3500.0), (-1050.0, 1750.0), (2450.0, 1750.0)]


@pytest.fixture(scope="module")
def pair():
    """One switched-off and one sharing engine for the single-level cases (gyp_search_level is never split over helper contexts)."""
    off, on = _engine(1), _engine(0)
    yield off, on
    off.close()
    on.close()


@pytest.mark.parametrize("center,spread", LEVELS)
def test_single_level_counts_equal_the_model(pair, center, spread):
    """Every state on one centre: each of the level's bins is one unit per stream, every cell reads a unit, none is left over; one
    satellite alone shares nothing.  Records byte-equal to the switched-off engine's."""
    off, on = pair
    n_bins = len(level_bins(center, spread))
    assert n_bins == 20
    for n_streams in (1, 6, 13):
        iq = _synth(13, 10)[: n_streams * 10 * N]
        for n_sats, ids in SAT_LISTS.items():
            want = off.search_level(iq, n_streams, 10, ids, center, spread)
            w_off = _witness(off)
            got = on.search_level(iq, n_streams, 10, ids, center, spread)
            w_on = _witness(on)
            where = (center, spread, n_streams, n_sats)
            assert got.tobytes() == want.tobytes(), where
            assert w_off == (0, 0, n_bins * n_sats * n_streams), (where, w_off)
            if n_sats == 1:
                assert w_on == (0, 0, n_bins * n_streams), (where, w_on)
            else:
                assert w_on == (n_bins * n_streams, n_bins * n_sats * n_streams, 0), (where, w_on)
            assert w_on == _single_level_model(center, spread, n_streams, n_sats, 10), where


def test_levels_below_the_third_and_other_rates_share_nothing(pair):
    """(350, 875) is a level-4 spread (875 * 4 < 7000), 4.092 Msps is not the 8-samples-per-chip kernel: no unit, every cell unshared."""
    _, on = pair
    iq = _synth(13, 10)
    on.search_level(iq, 13, 10, ALL_IDS, 350.0, 875.0)
    assert _witness(on) == (0, 0, len(level_bins(350.0, 875.0)) * 32 * 13)
    fs4, n4 = 4_092_000, 4092
    eng = _engine(0, fs4, n4)
    try:
        eng.search_level(_synth(3, 10, fs=fs4, n=n4), 3, 10, ALL_IDS, 0.0, 7000.0)
        assert _witness(eng) == (0, 0, 20 * 32 * 3)
        for name in WITNESS:                                   # read only
            with pytest.raises(_lib.GypsumHipError):
                eng.debug_set(name, 0)
    finally:
        eng.close()


def test_whole_scans_equal_the_model_fed_with_the_oracles_winners():
    """2 streams x 32 satellites and 2 streams x 3 satellites (where units of a single cell are common: they must stay on the unshared
    list).  Levels 1-3 go through plan_level / plan_units with the oracle's level winners as centres, levels 4-10 add every active cell
    to the unshared count; the device's three totals must equal the model's exactly, with the switch off as well."""
    _whole_scan_against_model([671000, 671001], ALL_IDS, label="2 x 32")
    per_level, _ = _whole_scan_against_model([671002, 671003], [31, 2, 17], label="2 x 3")
    assert per_level[1][2] + per_level[2][2] > 0, per_level      # the case is here for its single-cell units: there were some


@pytest.mark.parametrize("seed,params", [(672000, {"acq_reuse_level_records": 0.0}), (672001, {"acq_bins_per_spread": 7.0}),
                                         (672002, {"acq_bins_per_spread": 13.0}),
                                         (672003, {"acq_initial_spread_hz": 5000.0, "acq_min_spread_hz": 20.0})],
                         ids=["no_reuse", "bins7", "bins13", "spread5000"])
def test_whole_scan_counts_follow_the_tunables(seed, params):
    """One stream x 32 satellites with other gyp_params, the oracle's constants set to the same values in its worker processes.
    acq_bins_per_spread = 14 would fill all 28 bins of levels 1-3 but gyp_set_params refuses it (its fourth level, 875 Hz in steps of
    62, has 29 bins -- in the reference too): 13 is the largest value a whole scan admits, 27 bins at levels 1-3 and 28 below.  An
    initial spread of 5000 Hz needs acq_min_spread_hz = 20: at 10 the last level (19.5 Hz in steps of 1) has 40 bins and is refused as
    well.  Where level 3 asks for more than the 84 units per stream there is room for -- at 13 bins per spread it does -- the model
    caps and so must the device: the only place the 84-per-stream term of the room is reached."""
    per_level, room = _whole_scan_against_model([seed], ALL_IDS, params=params, label=str(params))
    if params.get("acq_bins_per_spread") == 13.0:      # steps of 538 / 269 / 134 Hz: level 3's grids no longer coincide (162 units wanted on the CPU)
        assert per_level[2][0] > room == 84, (per_level, room)
    print(f"[tunables {params}] level 3 asks for {per_level[2][0]} units, room {room}: the cap is {'' if per_level[2][0] > room else 'not '}reached")


def test_a_level_of_29_bins_is_refused():
    eng = _engine(0)
    try:
        with pytest.raises(_lib.GypsumHipError):
            eng.set_params(acq_bins_per_spread=14.0)
        with pytest.raises(_lib.GypsumHipError):
            eng.set_params(acq_initial_spread_hz=5000.0)
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. the 1 GiB cap, inside a stream
def test_the_spectra_cap_cuts_inside_a_stream():
    """n_ms = 40: 2^30 // (40 * 128 KiB) = 204 units.  Level 1 of 12 streams x 32 satellites asks for 240: streams 0-9 and the first
    four bins of stream 10 are shared, the other 36 bins' cells run on the unshared kernel in the same level.  Then whole scans of the
    same input, unsplit and in two parts of 6 streams (each part with its own 204): byte-equal, no cell lost or served twice, at most
    3 x 204 units per part.  (The oracle's trace of 384 forty-millisecond searches is not affordable here, so the whole scans are held
    to those invariants and not to exact counts.)"""
    n_streams, n_ms = 12, 40
    assert max_units_for(n_streams, 32, n_ms) == 204 == 2 ** 30 // (n_ms * 131072)
    iq = _synth(n_streams, n_ms, seed=40)
    off, on = _engine(1, no_acq_split=1), _engine(0, no_acq_split=1)
    try:
        want = off.search_level(iq, n_streams, n_ms, ALL_IDS, 0.0, 7000.0)
        w_off = _witness(off)
        got = on.search_level(iq, n_streams, n_ms, ALL_IDS, 0.0, 7000.0)
        w_on = _witness(on)
    finally:
        off.close()
        on.close()
    assert w_off == (0, 0, 240 * 32), w_off
    assert w_on == (204, 204 * 32, 36 * 32), w_on
    assert w_on == _single_level_model(0.0, 7000.0, n_streams, 32, n_ms)
    assert got.tobytes() == want.tobytes(), int(np.sum(got != want))
    for knobs, parts in (({"no_acq_split": 1}, 1), ({"acq_lanes": 2}, 2)):
        rec, w_on, w_off = _ab_scan(iq, n_streams, n_ms, ALL_IDS, **knobs)
        assert 204 < w_on[0] <= 3 * 204 * parts, (knobs, w_on)      # level 1 alone fills an unsplit scan's room
        assert sum(int(r["strength"] > 3.0) for r in rec) >= 4 * (n_streams - 1)
        print(f"[cap, whole scan {knobs}] {w_on} / switched off {w_off}")


# ------------------------------------------------------------------ 3. n_ms edges
@pytest.mark.parametrize("n_ms", [1, 2, 3, 21])
def test_n_ms_edges_are_byte_equal(n_ms):
    """The producer's prologue fetch (n_ms > 1) and its ms + 2 < n_ms fetch, the consumer's per-millisecond stride."""
    _, w_on, _ = _ab_scan(_synth(3, n_ms, seed=300 + n_ms), 3, n_ms, ALL_IDS)
    assert w_on[0] >= 3 * 20 + 3                                    # level 1's 20 units per stream and then some


@pytest.mark.parametrize("n_ms", [1, 2])
def test_one_and_two_milliseconds_against_the_oracle(n_ms):
    _whole_scan_against_model([673000 + n_ms], ALL_IDS, n_ms=n_ms, label=f"n_ms = {n_ms}")


# ------------------------------------------------------------------ 4. layouts
def test_strided_nan_guarded_layout_gives_the_packed_bytes():
    """13 streams at a stride of n_ms * N + 777 samples, NaN before, between and after them: the records of the packed layout and of
    the switched-off run, the input untouched."""
    n_streams, n_ms = 13, 10
    host = _synth(n_streams, n_ms)
    streams = [host[s * n_ms * N:(s + 1) * n_ms * N] for s in range(n_streams)]
    buf, stride = _guarded(streams, N, N, gap=777)
    assert stride == n_ms * N + 777
    packed, w_packed, _ = _ab_scan(host, n_streams, n_ms, ALL_IDS)
    for shared_off in (1, 0):
        eng = _engine(shared_off)
        try:
            d_iq = _dev_copy(eng, buf)
            d_out = eng.alloc(n_streams * 32 * ACQ_RESULT.itemsize)
            eng.acquire_dev(d_iq.ptr.value + N * 8, n_streams, stride, n_ms, ALL_IDS, d_out.ptr.value)
            w = _witness(eng)
            eng.sync()
            got = d_out.download(ACQ_RESULT, n_streams * 32)
            after = d_iq.download(np.complex64, buf.size)
        finally:
            eng.close()
        assert np.all(np.isfinite(got["strength"])) and np.all(np.isfinite(got["carrier_phase"]))
        assert got.tobytes() == packed.tobytes(), shared_off
        assert after.tobytes() == buf.tobytes(), shared_off
        if shared_off:
            _assert_off(w)
        else:
            assert w == w_packed, (w, w_packed)                     # the same units whatever the layout


# ------------------------------------------------------------------ 5. satellite lists
@pytest.mark.parametrize("ids", [[5], [7, 7], [31, 2, 17], list(range(1, 32))], ids=["one", "duplicate", "unsorted", "31"])
def test_satellite_lists(pair, ids):
    """A duplicate forms a two-cell unit of one satellite; an unsorted list and 31 of 32.  Level (0, 7000) with the model's counts, then
    a whole scan."""
    off, on = pair
    n_streams = 3
    iq = _synth(n_streams, 10, seed=500)
    want = off.search_level(iq, n_streams, 10, ids, 0.0, 7000.0)
    _assert_off(_witness(off))
    got = on.search_level(iq, n_streams, 10, ids, 0.0, 7000.0)
    assert got.tobytes() == want.tobytes()
    model = _single_level_model(0.0, 7000.0, n_streams, len(ids), 10)
    assert model == ((0, 0, 60) if len(ids) == 1 else (60, 60 * len(ids), 0))
    assert _witness(on) == model
    rec, _, _ = _ab_scan(iq, n_streams, 10, ids, shares=len(ids) > 1)
    if ids == [7, 7]:
        assert rec[0::2].tobytes() == rec[1::2].tobytes()             # the same satellite twice: the same record twice


# ------------------------------------------------------------------ 6. split scans inherit the switch
def test_helper_contexts_inherit_the_switch():
    """7 streams in parts of 2, 2 and 3 on the caller's context and two helpers.  With the switch at 1 no part shares -- the parent's
    counters include the helpers'.  With it at 0 the totals equal the unsplit scan's (rooms of 168 / 168 / 252 units split and 588
    unsplit, never reached: checked), and all four runs give the same bytes."""
    n_streams = 7
    iq = _synth(13, 10)
    runs, levels = {}, {}
    for shared_off in (1, 0):
        for label, knobs in (("split", {"acq_lanes": 3}), ("unsplit", {"no_acq_split": 1})):
            eng = _engine(shared_off, **knobs)
            try:
                runs[(shared_off, label)] = _scan(eng, iq, n_streams, 10, ALL_IDS)
                levels[(shared_off, label)] = _witness_levels(eng, 10)
            finally:
                eng.close()
    ref = runs[(1, "unsplit")][0]
    for key, (rec, w) in runs.items():
        assert rec.tobytes() == ref.tobytes(), key
        if key[0]:
            _assert_off(w, key)
            assert w[2] == runs[(1, "unsplit")][1][2], key
    w_split, w_unsplit = runs[(0, "split")][1], runs[(0, "unsplit")][1]
    assert w_split[0] > 0 and w_unsplit[0] > 7 * 20
    # no level of the unsplit scan filled its room of 588 (a part's own room is reached only if its streams average more than 84 units
    # at a level, against 70 at most in the model: then the totals could differ legitimately and this input would have to change)
    assert all(lv[0] < max_units_for(n_streams, 32, 10) == 588 for lv in levels[(0, "unsplit")]), levels[(0, "unsplit")]
    assert levels[(0, "split")] == levels[(0, "unsplit")], (levels[(0, "split")], levels[(0, "unsplit")])
    assert w_split == w_unsplit, (w_split, w_unsplit)
    assert w_split[1] + w_split[2] == runs[(1, "split")][1][2]
    assert all(lv[0] == 0 and lv[1] == 0 for lv in levels[(0, "split")][3:])       # levels 4-10 never share
    assert [lv[0] for lv in levels[(0, "split")][:1]] == [7 * 20]


# ------------------------------------------------------------------ 7. one context, many calls
def test_one_context_across_calls_of_different_sizes_and_rates():
    """A big scan, a tiny one, a long one, another rate, the first again, the switch flipped in between: each call's records and
    counters are what a fresh engine gives for that call alone (stale counts, unit lists laid out for another size, spectra of an
    earlier call would show)."""
    fs4, n4 = 4_092_000, 4092
    steps = [  # (fs, n, streams, n_ms, ids, switch)
        (FS, N, 13, 10, ALL_IDS, 0), (FS, N, 1, 2, [7, 19], 0), (FS, N, 5, 21, [31, 2, 17], 0), (fs4, n4, 3, 10, ALL_IDS, 0),
        (FS, N, 13, 10, ALL_IDS, 0), (FS, N, 13, 10, ALL_IDS, 1), (FS, N, 5, 21, [31, 2, 17], 0),
    ]
    eng = GypsumEngine(0)
    seen = []
    try:
        for fs, n, n_streams, n_ms, ids, shared_off in steps:
            host = _synth(n_streams, n_ms, fs=fs, n=n)
            if eng.fs != fs:
                eng.set_stream_format(fs, n)
            eng.debug_set("no_acq_shared_fwd", shared_off)
            got, w = _scan(eng, host, n_streams, n_ms, ids, n=n)
            fresh = _engine(shared_off, fs, n)
            try:
                want, w_fresh = _scan(fresh, host, n_streams, n_ms, ids, n=n)
            finally:
                fresh.close()
            where = (fs, n_streams, n_ms, len(ids), shared_off)
            assert got.tobytes() == want.tobytes(), where
            assert w == w_fresh, (where, w, w_fresh)
            assert (w[0] > 0) == (fs == FS and not shared_off), (where, w)
            seen.append(w)
    finally:
        eng.close()
    assert seen[0] == seen[4] and seen[2] == seen[6] and seen[5][:2] == (0, 0) and seen[5][2] == seen[0][1] + seen[0][2], seen


# ------------------------------------------------------------------ 8. other launch geometries
def test_reserved_compute_units_change_nothing():
    """cells_cu_reserve changes the producer's and the consumer's grids and the unit-to-XCD mapping: the same bytes and the same units."""
    iq = _synth(13, 10)
    ref = None
    for reserve in (0, 64, 128):
        rec, w_on, _ = _ab_scan(iq, 13, 10, ALL_IDS, cells_cu_reserve=reserve)
        if ref is None:
            ref = (rec, w_on)
        assert rec.tobytes() == ref[0].tobytes(), reserve
        assert w_on == ref[1], reserve
    assert active_cells(plan_level(np.zeros((13, 32)), 7000.0, None)) == 13 * 32 * 20 and MAX_BINS == 28
