"""The sample path's launch plan at the grid's height limit (csrc/resample_plan.hpp; tests/test_host_sanitizers.py sweeps the plan
itself on the CPU): 65536 streams are refused before anything is launched or written, through both resampling entries, and 65535
streams -- the last legal grid.y -- run and give what a degenerate window gives at any height, exact zeros everywhere."""
from __future__ import annotations

import numpy as np
import pytest

from gypsum_amd import _lib
from gypsum_amd.engine import GypsumEngine
from gypsum_amd.packing import Packing

pytestmark = pytest.mark.gpu

FS_IN, FS_OUT, N_OUT = 2_048_000, 2_046_000, 2046
MARKER = np.complex64(-7.25 + 3.5j)


@pytest.fixture(scope="module")
def eng():
    e = GypsumEngine(0)
    e.set_stream_format(FS_OUT, N_OUT)
    yield e
    e.close()


def test_65536_streams_are_refused_and_nothing_is_written(eng):
    """n_streams = 65536 with an empty window and a NULL input passes the argument check and is refused by the plan (grid.y would be
    65536): GYP_E_BAD_ARG with the launch's own text, and the 8 bytes of output keep their marker."""
    marker = np.array([MARKER])
    d_out = eng.alloc(marker.nbytes).upload(marker)
    calls = [lambda: eng.resample_iq_dev(_lib.GYP_FMT_I8, None, 65536, 0, 0, 0, 1.0, FS_IN, 32, 0, 1, N_OUT, d_out.ptr.value),
             lambda: eng.resample_packed_dev(Packing(2, (-3.0, -1.0, 1.0, 3.0)), None, 65536, 0, 0, 0, 0, 1.0, FS_IN, 0, 32, 0, 1, N_OUT, d_out.ptr.value)]
    for call in calls:
        with pytest.raises(_lib.GypsumHipError) as e:
            call()
        assert e.value.code == _lib.GYP_E_BAD_ARG and "gyp_resample: launch too large (split it)" in str(e.value)
        eng.sync()
        assert d_out.download(np.complex64, 1)[0] == MARKER
    d_out.free()


def test_65535_streams_of_an_empty_window_are_all_zero(eng):
    """The last legal grid height: 65535 streams x one millisecond of an empty window over an output full of markers.  Every output
    sample is exactly zero -- checked on the device, by the per-millisecond statistics (sum of squares and largest magnitude 0)."""
    n_streams = 65535
    d_out = eng.alloc(n_streams * N_OUT * 8)
    d_out.upload(np.full(n_streams * N_OUT, MARKER))
    d_stats = eng.alloc(n_streams * _lib.IQ_STATS.itemsize)
    eng.iq_stats_dev(d_out.ptr.value, n_streams, N_OUT, 1, N_OUT, 0.0, d_stats.ptr.value)
    before = d_stats.download(_lib.IQ_STATS, n_streams)
    assert (before["max_abs"] == np.float32(7.25)).all()                        # the statistics see every stream's marker
    eng.resample_iq_dev(_lib.GYP_FMT_I8, None, n_streams, 0, 0, 0, 1.0, FS_IN, 32, 0, 1, N_OUT, d_out.ptr.value)
    eng.iq_stats_dev(d_out.ptr.value, n_streams, N_OUT, 1, N_OUT, 0.0, d_stats.ptr.value)
    after = d_stats.download(_lib.IQ_STATS, n_streams)
    d_out.free()
    d_stats.free()
    assert (after["sum_sq"] == 0.0).all() and (after["max_abs"] == 0.0).all() and (after["sum_re"] == 0.0).all() and (after["sum_im"] == 0.0).all()
