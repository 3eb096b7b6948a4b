"""The second and later launches of one conditioning call.  Every stage takes a fixed number of streams per launch (their
parameters travel by value in a kernel argument: 8 levels, 8 tone lists, 8 blankers, 8 centres) and a call of more streams is cut
into chunks; the statistics kernel takes every (stream, millisecond) in one launch.  Here 9 streams make a second chunk of one stream
and 17 a third, with parameters that differ from stream to stream, so a chunk that read another chunk's samples, parameters or
output rows cannot pass.  The models, bounds and array constructors are those of the stages' own test modules."""
from __future__ import annotations

import numpy as np
import pytest

import blank_model
from gypsum_amd.engine import GypsumEngine
from gypsum_amd.level import STATS_DTYPE, IqLevel
from test_gpu_blank import _hist, _pulsed
from test_gpu_level import _condition, _int_samples, _numpy_condition, _same, _stats
from test_gpu_notch import _assert_notched_within_bound, _notch, _signal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = GypsumEngine(0)
    e.set_stream_format(2_046_000, 2046)
    yield e
    e.close()


@pytest.mark.parametrize("stride", [2 * 1023 + 2, 2 * 1023 + 3], ids=["even stride", "odd stride"])
def test_seventeen_levels_condition_their_own_streams(eng, stride):
    """17 streams of 2 x 1023 + 1 samples: three launches (8, 8, 1).  An even stride from an aligned base takes 16-byte accesses,
    an odd one 8-byte accesses; the results are numpy's float32 (x - dc) * g bit for bit, and nothing else is written."""
    n_streams, n_samples = 17, 2 * 1023 + 1
    rng = np.random.default_rng(stride)
    flat = (rng.standard_normal(n_streams * stride) * 40 + 128 + 1j * (rng.standard_normal(n_streams * stride) * 40 + 127)).astype(np.complex64)
    levels = [IqLevel(100.0 + 3.0 * s, 130.0 - 2.5 * s, float(np.float32(0.01 * (s + 1)))) for s in range(n_streams)]
    for in_place in (False, True):
        out, src = _condition(eng, flat, 0, n_streams, stride, n_samples, levels, in_place)
        touched = np.zeros(flat.size, dtype=bool)
        for s, level in enumerate(levels):
            a = s * stride
            assert _same(out[a:a + n_samples], _numpy_condition(flat[a:a + n_samples], level)), (in_place, s)
            touched[a:a + n_samples] = True
        if in_place:
            assert _same(out[~touched], flat[~touched])
        else:
            assert np.isnan(out[~touched].real).all() and _same(src, flat)


NOTCH_LISTS = [[], [100_300], [100_300, -203_000]]
NOTCH_AMPS = [[], [5.0], [5.0, 0.5]]


@pytest.mark.parametrize("n_streams", [9, 17])
def test_streams_of_many_launches_are_notched_with_their_own_lists(eng, n_streams):
    """n = 1023, 2 ms; stream s carries s % 3 tones, so every chunk holds empty lists beside full ones.  Within the notch tests' own
    bound of the float64 model; the empty lists return the input bits; the same bits with the residual kept in the output buffer."""
    n, n_ms, fs, first = 1023, 2, 1_023_000, 2 ** 40 + 17
    stride = n_ms * n + 3
    rng = np.random.default_rng(n_streams)
    flat = (rng.standard_normal(1 + n_streams * stride) + 1j * rng.standard_normal(1 + n_streams * stride)).astype(np.complex64)
    lists = [NOTCH_LISTS[s % 3] for s in range(n_streams)]
    for s in range(n_streams):
        a = 1 + s * stride
        flat[a:a + n_ms * n] = _signal(rng, n_ms * n, fs, first, list(zip(lists[s], NOTCH_AMPS[s % 3])), 0.05 * (1 + s))
    out, src = _notch(eng, flat, 1, n_streams, stride, first, n_ms, n, fs, lists, False)
    touched = np.zeros(flat.size, dtype=bool)
    for s in range(n_streams):
        a = 1 + s * stride
        touched[a:a + n_ms * n] = True
        _assert_notched_within_bound(out[a:a + n_ms * n], flat[a:a + n_ms * n], fs, n, lists[s], first, f"{n_streams} streams, stream {s}")
        if not lists[s]:
            assert _same(out[a:a + n_ms * n], flat[a:a + n_ms * n]), s
    assert np.isnan(out[~touched].real).all() and _same(src, flat)
    if n_streams == 17:
        try:
            eng.debug_set("notch_no_lds", 1)
            other, _ = _notch(eng, flat, 1, n_streams, stride, first, n_ms, n, fs, lists, False)
        finally:
            eng.debug_set("notch_no_lds", 0)
        assert _same(other[touched], out[touched])


def test_nine_histograms_about_their_own_centres(eng):
    """9 streams of 2046 samples: two launches (8, 1); the integers of blank_model.hist about each stream's centre."""
    n_streams, n_samples = 9, 2046
    stride = n_samples + 3
    flat = _pulsed(1 + n_streams * stride, 9)
    centres = [complex(0.25 * s, -0.125 * s) for s in range(n_streams)]
    got = _hist(eng, flat, 1, n_streams, stride, n_samples, np.array([[c.real, c.imag] for c in centres]))
    want = np.stack([blank_model.hist(flat[1 + s * stride:1 + s * stride + n_samples], centres[s]) for s in range(n_streams)])
    assert want.sum(axis=1).tolist() == [n_samples] * n_streams and len({w.tobytes() for w in want}) == n_streams
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))


def test_statistics_of_nine_streams_in_one_call_are_each_streams_own(eng):
    """9 streams x 3 ms of n = 1023 in one call against one call per stream, bit for bit."""
    n_streams, n_ms, n = 9, 3, 1023
    stride = n_ms * n + 3
    flat = _int_samples(np.random.default_rng(93), 1 + n_streams * stride, 32767)
    got = _stats(eng, flat, 1, n_streams, stride, n_ms, n, 30000.0)
    assert got.shape == (n_streams, n_ms) and got.dtype == STATS_DTYPE
    for s in range(n_streams):
        assert _same(_stats(eng, flat, 1 + s * stride, 1, 0, n_ms, n, 30000.0)[0], got[s]), s
    assert len({got[s].tobytes() for s in range(n_streams)}) == n_streams
