"""Shared forward transforms of the acquisition search (gyp_debug_set "no_acq_shared_fwd"): at 8.184 Msps the first three levels
of a scan run the wipe-off and the 8 forward transforms once per (stream, Doppler bin) and every satellite on that bin reads the
spectra back.  The spectra are the values the unshared kernel multiplies, so every record must be byte for byte what the unshared
path gives: whole scans (split over helper contexts and not), single levels at level-2 and level-3 centres, and a scan of one
stream and one satellite where nothing is shared."""
from __future__ import annotations

import numpy as np
import pytest

from acq_units_model import level_bins
from gypsum_amd._lib import ACQ_RESULT, SYNTH_SAT
from gypsum_amd.engine import GypsumEngine

pytestmark = pytest.mark.gpu
FS, N = 8_184_000, 8184
ALL_IDS = list(range(1, 33))
N_MS = 10


def _scene(rng, n_streams):
    """Six planted satellites per stream (the other 26 are noise only), one stream with none at all."""
    sats = np.zeros((n_streams, 6), dtype=SYNTH_SAT)
    for s in range(n_streams):
        sats[s]["sat_id"] = rng.choice(np.arange(1, 33), size=6, replace=False)
        sats[s]["code_phase"] = rng.integers(0, N, 6)
        sats[s]["doppler_hz"] = rng.uniform(-6500, 6500, 6)
        sats[s]["carrier_phase"] = rng.uniform(0, 2 * np.pi, 6)
        sats[s]["amplitude"] = 0.0 if s == n_streams - 1 else 40.0 / N
        sats[s]["nav_bit_offset_ms"] = rng.integers(0, 20, 6)
    return sats


def _engine(shared_off, **knobs):
    eng = GypsumEngine(0)
    eng.set_stream_format(FS, N)
    eng.debug_set("no_acq_shared_fwd", shared_off)
    for k, v in knobs.items():
        eng.debug_set(k, v)
    assert eng.debug_get("no_acq_shared_fwd") == shared_off
    return eng


@pytest.fixture(scope="module")
def samples():
    """13 streams x 10 ms, generated once on the device and kept on the host."""
    rng = np.random.default_rng(2026)
    n_streams = 13
    gen = GypsumEngine(0)
    gen.set_stream_format(FS, N)
    stride = N_MS * N
    iq = gen.alloc(n_streams * stride * 8)
    gen.synth_iq(iq, n_streams, stride, N_MS, _scene(rng, n_streams), 6 * 40.0 / N, 4242)
    host = iq.download(np.complex64, n_streams * stride)
    gen.close()
    return host, n_streams


def _witness(eng):
    """(units given a forward pass of their own, cells that read a unit's spectra, cells on the unshared list) of the last search."""
    return tuple(int(eng.debug_get(k)) for k in ("last_acq_units", "last_acq_shared_cells", "last_acq_unshared_cells"))


def _scan(eng, host, n_streams, sat_ids):
    stride = N_MS * N
    buf = eng.alloc(n_streams * stride * 8)
    buf.upload(host[: n_streams * stride])
    out = eng.alloc(n_streams * len(sat_ids) * ACQ_RESULT.itemsize)
    eng.acquire_dev(buf.ptr.value, n_streams, stride, N_MS, sat_ids, out.ptr.value)
    eng.sync()
    return out.download(ACQ_RESULT, n_streams * len(sat_ids))


@pytest.mark.parametrize("knobs", [{}, {"no_acq_split": 1}, {"acq_lanes": 4}], ids=["two_lanes", "unsplit", "four_lanes"])
def test_shared_forward_scan_is_byte_equal(samples, knobs):
    host, n_streams = samples
    ref_eng, eng = _engine(1, **knobs), _engine(0, **knobs)
    want = _scan(ref_eng, host, n_streams, ALL_IDS)
    got = _scan(eng, host, n_streams, ALL_IDS)
    assert got.tobytes() == want.tobytes(), int(np.sum(got != want))
    assert sum(int(r["strength"] > 3.0) for r in want) >= 4 * (n_streams - 1)   # the planted satellites are found
    w_off, w_on = _witness(ref_eng), _witness(eng)                               # (helper contexts included)
    assert w_off[0] == 0 and w_off[1] == 0, w_off
    assert w_on[0] >= 20 * n_streams and w_on[1] >= 20 * 32 * n_streams, w_on   # level 1 alone: 20 units per stream, every cell shared
    assert w_on[1] + w_on[2] == w_off[2], (w_on, w_off)                         # no cell lost, none served twice
    ref_eng.close()
    eng.close()


def test_one_stream_one_satellite_shares_nothing_and_matches(samples):
    host, _ = samples
    for sats in ([7], [7, 19]):
        ref_eng, eng = _engine(1), _engine(0)
        want = _scan(ref_eng, host, 1, sats)
        got = _scan(eng, host, 1, sats)
        assert got.tobytes() == want.tobytes(), sats
        assert _witness(ref_eng)[:2] == (0, 0)
        if len(sats) == 1:
            assert _witness(eng)[:2] == (0, 0) and _witness(eng)[2] == _witness(ref_eng)[2]      # [7] shares nothing
        else:
            assert int(eng.debug_get("last_acq_units_l1")) == 20 and _witness(eng)[0] >= 20        # [7, 19]: level 1's 20 bins, two cells each
            assert int(eng.debug_get("last_acq_shared_cells_l1")) == 40
        ref_eng.close()
        eng.close()


@pytest.mark.parametrize("center,spread", [(-2100.0, 3500.0), (1400.0, 3500.0), (-1050.0, 1750.0), (2450.0, 1750.0), (350.0, 875.0)])
def test_single_levels_at_level_2_and_3_centres_are_byte_equal(samples, center, spread):
    """gyp_search_level_dev with every satellite on one grid: the level's winners, their code phases and float64 strengths.
    (350, 875) is a level-4 spread -- 875 * 4 < 7000 -- and never enters the shared branch: there the two engines run the same
    kernel, and the witness must say so (no unit); the other four share every cell."""
    host, n_streams = samples
    ref_eng, eng = _engine(1), _engine(0)
    iq = host[: n_streams * N_MS * N]
    want = ref_eng.search_level(iq, n_streams, N_MS, ALL_IDS, center, spread)
    got = eng.search_level(iq, n_streams, N_MS, ALL_IDS, center, spread)
    assert got.tobytes() == want.tobytes(), int(np.sum(got != want))
    n_bins = len(level_bins(center, spread))                  # 20, and 21 for (350, 875): range(-525, 1225, 87)
    assert _witness(ref_eng) == (0, 0, n_bins * 32 * n_streams)
    if spread * 4 < 7000.0:
        assert _witness(eng) == (0, 0, n_bins * 32 * n_streams)
    else:
        assert _witness(eng) == (n_bins * n_streams, n_bins * 32 * n_streams, 0)
    ref_eng.close()
    eng.close()


def test_knob_is_range_checked_and_read_back():
    from gypsum_amd._lib import GypsumHipError
    eng = GypsumEngine(0)
    eng.set_stream_format(FS, N)
    assert eng.debug_get("no_acq_shared_fwd") == 0
    for bad in (2, -1, 0.5, float("nan")):
        with pytest.raises(GypsumHipError):
            eng.debug_set("no_acq_shared_fwd", bad)
    eng.debug_set("no_acq_shared_fwd", 1)
    assert eng.debug_get("no_acq_shared_fwd") == 1
    eng.close()
