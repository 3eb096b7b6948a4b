"""What each measurement of an ingest handle sees: the handle's output behind the stages in front of the one measured, whatever else
is installed.  The chain is producer -> blanker -> excisor -> notches -> level, and find_pulses, find_excisor, find_tones and
calibrate measure in front of the blanker, the excisor, the notches and the level.

One recording of 10 ms at 2.046 Msps (int8, block_ms = 3: blocks of 3, 3, 3 and 1 ms) with pulses, a frequency-modulated
interferer and a CW tone.  Handle A has all four stages installed with fixed values; for each stage X a handle B_X has only the
stages in front of X.  A's measurement of X equals B_X's exactly -- the kernels, their inputs and the host arithmetic are the
same -- and, for every X behind the blanker, differs from a bare handle's, so the stages in front of X were indeed applied."""
from __future__ import annotations

import numpy as np
import pytest

import blank_model
import excise_model
import notch_model
from gypsum_amd import synth
from gypsum_amd.blanker import Blanker
from gypsum_amd.engine import GypsumEngine
from gypsum_amd.excisor import Excisor
from gypsum_amd.ingest import IqFileIngest
from gypsum_amd.level import IqLevel

pytestmark = pytest.mark.gpu

FS, N, N_MS, BLOCK_MS = notch_model.SCENE_FS, notch_model.SCENE_N, 10, 3
TONE_HZ = -403_000
# in int8 words: the scene's largest component is 120, its noise about 0.85 per component, the tone and the interferer about 8.5 each
BLANKER, EXCISOR, LEVEL = Blanker(0.0, 0.0, 30.0, 4), Excisor(100.0, 1), IqLevel(0.25, -0.5, 0.03125)
STAGES = ("blanker", "excisor", "notches", "level")     # the chain's order


@pytest.fixture(scope="module")
def eng():
    e = GypsumEngine(0)
    e.set_stream_format(FS, N)
    yield e
    e.close()


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    x, _ = notch_model.scene(N_MS, tone_hz=(TONE_HZ,), tone_db=(20.0,))
    _, sigma = synth.default_amplitudes(FS)
    x = x.astype(np.complex128) + 0.1 * excise_model.jammer("fm", len(x), sigma) + blank_model.pulses(len(x), sigma, blank_model.PULSE_SEED)
    w8, _, _ = notch_model.scene_words(x.astype(np.complex64))
    path = tmp_path_factory.mktemp("chain") / "chain.i8"
    np.concatenate([w8, np.zeros(2, np.int8)]).tofile(path)
    return path


def _install(ing, stages):
    if "blanker" in stages:
        ing.set_blanker(BLANKER)
    if "excisor" in stages:
        ing.set_excisor(EXCISOR)
    if "notches" in stages:
        ing.set_notches([TONE_HZ])
    if "level" in stages:
        ing.set_level(LEVEL)


def _installed(ing):
    return ing.blanker, ing.get_excisor(), ing.notches, ing.level


def _measure(ing, stage):
    """What the measurement in front of `stage` returns; nothing is left installed that was not."""
    if stage == "blanker":
        return ing.find_pulses(install=False)
    if stage == "excisor":
        return ing.find_excisor(install=False)
    if stage == "notches":
        return ing.find_tones(install=False)
    before = ing.level
    found = ing.calibrate(n_ms=N_MS)          # measures and installs
    ing.set_level(before)
    return found


def test_each_measurement_sees_the_stages_in_front_of_it_and_nothing_else(eng, recording):
    def open_with(stages):
        ing = IqFileIngest(recording, FS, np.int8, block_ms=BLOCK_MS, depth=3, engine=eng)
        _install(ing, stages)
        return ing

    want, bare = {}, {}
    for i, stage in enumerate(STAGES):
        for into, stages in ((want, STAGES[:i]), (bare, ())):
            ing = open_with(stages)
            try:
                into[stage] = _measure(ing, stage)
            finally:
                ing.close()
    a = open_with(STAGES)
    try:
        assert a.total_ms == N_MS
        full = (Blanker.from_record(BLANKER.record()), Excisor.from_record(EXCISOR.record()), [TONE_HZ], IqLevel.from_record(LEVEL.record()))
        assert _installed(a) == full
        cursor = 0
        for stage in STAGES:
            got = _measure(a, stage)
            print(stage, got, want[stage], bare[stage])
            assert got == want[stage], stage
            if stage != "blanker":
                assert got != bare[stage], stage          # the stages in front did something to what was measured
            assert _installed(a) == full, stage
            first, n_ms, _ = a.next_device_block()    # the cursor is where it was
            assert (first, n_ms) == (cursor, min(BLOCK_MS, N_MS - cursor)), stage
            cursor += n_ms
        assert cursor == N_MS and a.next_device_block() is None
        eng.sync()
    finally:
        a.close()
