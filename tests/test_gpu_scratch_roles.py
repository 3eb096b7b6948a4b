"""The host-buffer entry points of one context called in turn, at growing and shrinking shapes, and a bank whose buffers grow.

Every entry point stages its inputs and results in device buffers the context (or the bank) owns and grows on demand.  What is
checked here, through the public GypsumEngine API only: a call's result does not depend on which calls the same context made
before it, at which shapes.  Each result is compared byte for byte (tobytes()) with the same call on a fresh engine that has made
no other call.  That catches an entry point and the device function it calls sharing a buffer, a stale capacity after a buffer
has grown, and a sub-array of a shared buffer that moved.  No call needed a tolerance: all of them are bit-reproducible.

All of it runs at 2.046 Msps (2 samples per chip), the smallest rate that also takes the speculative tracking path.
"""
from __future__ import annotations

import numpy as np
import pytest

from gypsum_amd import _lib, synth
from gypsum_amd.engine import GypsumEngine

pytestmark = pytest.mark.gpu

FS, N = 2_046_000, 2046
# the second at least twice the first in every dimension: doubling defeats the 25 % growth slack, so every buffer is reallocated
SMALL = dict(n_streams=1, n_ms=2, n_sats=2, n_bins=3, n_cells=4)
LARGE = dict(n_streams=3, n_ms=5, n_sats=5, n_bins=7, n_cells=40)
CALLS = ("correlate_cells", "correlate_grid", "search_level", "acquire", "track_step", "track_block", "synth_iq")


def _engine() -> GypsumEngine:
    eng = GypsumEngine(0)
    eng.set_stream_format(FS, N)
    return eng


def _times(first_ms: int, n_ms: int):
    return [round((first_ms + i) * N / FS, 6) for i in range(n_ms)]


def _inputs(shape, seed):
    n_streams, n_ms, n_sats, n_bins, n_cells = (shape[k] for k in ("n_streams", "n_ms", "n_sats", "n_bins", "n_cells"))
    scenes = [synth.random_scene(FS, n_ms, n_sats, seed + 10 * s) for s in range(n_streams)]
    iq = np.concatenate([synth.render(sc) for sc in scenes])
    ids = [s.sat_id for s in scenes[0].sats]
    cells = np.zeros(n_cells, dtype=_lib.CELL_DESC)
    chans = np.zeros(n_sats, dtype=_lib.CHAN_IN)
    inits = np.zeros(3, dtype=_lib.CHAN_INIT)
    for i in range(n_cells):
        sat = scenes[i % n_streams].sats[i % n_sats]
        cells[i] = (i % n_streams, sat.sat_id, round(sat.doppler_hz) + 25.0 * (i // n_sats), (i * 37) % N, 0)
    for i in range(n_sats):
        sat = scenes[i % n_streams].sats[i]
        chans[i] = (i % n_streams, sat.sat_id, round(sat.doppler_hz), sat.carrier_phase, sat.code_phase, 0)
    for i in range(3):
        sat = scenes[i % n_streams].sats[i % n_sats]
        inits[i] = (i % n_streams, sat.sat_id, round(sat.doppler_hz), sat.carrier_phase, sat.code_phase, 0)
    synth_sats = np.zeros((n_streams, n_sats), dtype=_lib.SYNTH_SAT)
    for s, sc in enumerate(scenes):
        for i, sat in enumerate(sc.sats):
            synth_sats[s, i] = (sat.sat_id, sat.code_phase, sat.doppler_hz, sat.carrier_phase, sat.amplitude, sat.nav_bit_offset_ms)
    return dict(shape, iq=iq, ids=ids, bins=np.linspace(-3000.0, 3000.0, n_bins), cells=cells, chans=chans, inits=inits,
                first_ms=np.ascontiguousarray(iq.reshape(n_streams, n_ms, N)[:, 0, :]), synth_sats=synth_sats, seed=seed)


def _call(eng: GypsumEngine, name: str, x) -> bytes:
    """One host-buffer entry point on `eng`; everything it returned, as bytes."""
    ns, n_ms = x["n_streams"], x["n_ms"]
    if name == "correlate_cells":
        out, prof = eng.correlate_cells(x["iq"], ns, n_ms, x["cells"], _lib.GYP_NON_COHERENT, want_profiles=True)
        return out.tobytes() + prof.tobytes()
    if name == "correlate_grid":
        return eng.correlate_grid(x["iq"], ns, n_ms, x["ids"], x["bins"], _lib.GYP_NON_COHERENT).tobytes()
    if name == "search_level":
        return eng.search_level(x["iq"], ns, n_ms, x["ids"], 0.0, 7000.0).tobytes()
    if name == "acquire":
        return eng.acquire(x["iq"], ns, n_ms, x["ids"]).tobytes()
    if name == "track_step":
        out, prof = eng.track_step(x["first_ms"], ns, _times(0, ns), x["chans"], want_profiles=True)
        return out.tobytes() + prof.tobytes()
    if name == "track_block":
        bank = eng.create_bank(x["inits"])
        rec = bank.track_block(x["iq"], ns, n_ms, _times(0, n_ms))
        state = bank.state()
        bank.close()
        return rec.tobytes() + b"".join(state[k].tobytes() for k in sorted(state))
    assert name == "synth_iq"
    buf = eng.alloc(ns * n_ms * N * 8)
    eng.synth_iq(buf, ns, n_ms * N, n_ms, x["synth_sats"], 0.05, x["seed"])
    out = buf.download(np.complex64, ns * n_ms * N)
    buf.free()
    return out.tobytes()


@pytest.fixture(scope="module")
def cases():
    """(inputs, {call: result on a fresh engine that makes no other call}) for the small and the large shapes."""
    made = []
    for shape, seed in ((SMALL, 4100), (LARGE, 4200)):
        x = _inputs(shape, seed)
        alone = {}
        for name in CALLS:
            eng = _engine()
            alone[name] = _call(eng, name, x)
            eng.close()
        made.append((x, alone))
    return made


def test_results_do_not_depend_on_the_calls_before(cases):
    """correlate_cells, correlate_grid, search_level, acquire, track_step, track_block, synth_iq on ONE engine: at the small
    shapes, at shapes more than twice as large, at the small shapes again."""
    small, large = cases
    eng = _engine()
    for round_name, (x, alone) in (("small", small), ("large", large), ("small again", small)):
        for name in CALLS:
            got = _call(eng, name, x)
            assert len(got) == len(alone[name]) and len(got) > 0
            assert got == alone[name], f"{name} ({round_name}) differs from the same call on a fresh engine"
    eng.close()
    # the results are not trivially equal: the two shapes, and the calls among themselves, return different bytes
    assert len({alone[name] for _, alone in cases for name in CALLS}) == 2 * len(CALLS)


def _bank_sequence():
    """3 channels on planted satellites: blocks of 8, 300 (four sub-blocks: the checkpoint, history and round buffers grow) and
    8 ms, then kept profiles switched 0 -> 2 -> 4 -> 0 with a block of 8 ms behind each."""
    first, cuts = 9, (8, 300, 8, 8, 8, 8)
    n_ms = first + sum(cuts)
    scene = synth.random_scene(FS, n_ms, 3, 4300)
    iq = synth.render(scene)
    rng = np.random.default_rng(4301)
    inits = np.zeros(3, dtype=_lib.CHAN_INIT)
    for i, s in enumerate(scene.sats):
        inits[i] = (0, s.sat_id, float(int(round(s.doppler_hz)) + int(rng.integers(-2, 3))),
                    float(np.angle(np.exp(1j * (s.carrier_phase + rng.uniform(-0.2, 0.2))))), s.code_phase, 0)
    return iq, inits, first, cuts


def _run_bank(eng, iq, inits, first, cuts):
    bank = eng.create_bank(inits)
    records, rows = [], []
    at = first
    for step, cut in enumerate(cuts):
        if step >= 3:
            bank.keep_profiles((2, 4, 0)[step - 3])
        records.append(bank.track_block(iq[at * N:(at + cut) * N], 1, cut, _times(at, cut)))
        at += cut
        if step >= 3:
            rows.append([bank.profiles(c) for c in range(len(inits))])
    state = bank.state()
    bank.close()
    return records, rows, state


def test_a_bank_whose_buffers_grow_tracks_like_a_fresh_one():
    iq, inits, first, cuts = _bank_sequence()
    eng = _engine()
    got_rec, got_rows, got_state = _run_bank(eng, iq, inits, first, cuts)
    eng.close()
    fresh = _engine()
    want_rec, want_rows, want_state = _run_bank(fresh, iq, inits, first, cuts)
    fresh.close()
    for step, (a, b) in enumerate(zip(got_rec, want_rec)):
        assert a.shape == (3, cuts[step]) and a.tobytes() == b.tobytes(), f"block {step} ({cuts[step]} ms)"
    for depth, a, b in zip((2, 4, 0), got_rows, want_rows):
        for c in range(3):
            assert a[c].shape == (depth, N) and a[c].tobytes() == b[c].tobytes(), f"kept profiles, depth {depth}, channel {c}"
    for k in want_state:
        assert got_state[k].tobytes() == want_state[k].tobytes(), k
    # the planted satellites are tracked, not lost: the records carry signal
    assert not got_state["lost"].any() and all((r["status"] == 0).all() for r in got_rec)
