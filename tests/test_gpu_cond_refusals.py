"""Every refused call of the conditioning stages and of the ingest calls that drive them, with its return code and the text
gyp_last_error gives: gyp_iq_stats_dev, gyp_condition_iq_dev, gyp_iq_tones_dev, gyp_notch_iq_dev, gyp_blank_iq_dev,
gyp_iq_power_hist_dev, gyp_excise_iq_dev, gyp_iq_spectrum_hist_dev, gyp_track_quality_dev and gyp_ingest_set_* / get_* / calibrate /
find_tones / find_pulses / find_excisor / last_blanked / last_excised / next_host.

One table (refused_calls), one row per condition: where an `if` tests several conditions, each has a row of its own.  The expected
(code, text) pairs are tests/golden/cond_refusals.json, recorded once from the library as it stood before these entry points' checks
were gathered into shared helpers; the test reads the file and never writes it.  Before every row the error text of the context
(and the thread's text behind gyp_last_error(NULL)) is set to a sentinel by another refused call, so a row that returned a code
without a text of its own would show the sentinel.

Not in the table: gyp_ingest_find_tones' refusal of a rate outside [1000, 2^31) Hz -- no handle can be opened at such a rate (the
range check in front of it needs a recording of at least one millisecond at 2^31 Hz) -- and refusals that come from HIP itself."""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from gypsum_amd import _lib
from gypsum_amd.engine import GypsumEngine

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "cond_refusals.json"
FS, N = 2_046_000, 2046
INF, NAN = float("inf"), float("nan")


def _level(dc_re=0.0, dc_im=0.0, gain=1.0, reserved=0):
    r = np.zeros(1, dtype=_lib.IQ_LEVEL)
    r[0] = (dc_re, dc_im, gain, reserved)
    return r


def _blanker(center_re=0.0, center_im=0.0, threshold=3.0, guard=4):
    r = np.zeros(1, dtype=_lib.BLANKER)
    r[0] = (center_re, center_im, threshold, guard)
    return r


def _excisor(threshold=3.0, guard=2, reserved=(0, 0)):
    r = np.zeros(1, dtype=_lib.EXCISOR)
    r[0] = (threshold, guard, reserved)
    return r


def _tones(freqs=(), count=None, reserved=0, n=1):
    r = np.zeros(n, dtype=_lib.NOTCH_TONES)
    for row in r:
        row["count"] = len(freqs) if count is None else count
        row["reserved"] = reserved
        row["freq_hz"][:len(freqs)] = freqs
    return r


def _i64(values):
    return np.array(values, dtype=np.int64)


class Env:
    """A context, a device buffer, and the handles the ingest rows need: `dev` (40 ms of int8 noise at 2.046 Msps on the context),
    `zeros` (the same length of zero words), `slow` (1200 ms at 1000 Hz: 1000 ms of it hold 1000 samples), `wide` (2 ms at
    65.537 Msps: more samples per millisecond than the blanker takes), `host` (opened without a context), `chain` (as `dev`: the
    handle whose stages gyp_ingest_next_host's rows switch on and off again), `resampled` (the same file read as 4.092 Msps) and
    `packed` (the same file read as 2-bit I,Q words at the context's rate)."""

    def __init__(self, tmp: Path) -> None:
        self.eng = GypsumEngine(0)
        self.eng.set_stream_format(FS, N)
        self.lib, self.ctx = self.eng.lib, self.eng.ctx
        self.buf = self.eng.alloc(1 << 16)
        self.p = self.buf.ptr.value
        rng = np.random.default_rng(7)
        files = {"dev": (rng.integers(-100, 101, 2 * (40 * N + 1)).astype(np.int8), FS, N, 5),
                 "zeros": (np.zeros(2 * (40 * N + 1), dtype=np.int8), FS, N, 5),
                 "slow": (rng.integers(-100, 101, 2 * 1201).astype(np.int8), 1000, 1, 50),
                 "wide": (np.zeros(2 * (2 * 65537 + 1), dtype=np.int8), 65_537_000, 65537, 1)}
        self.handles = {}
        for name, (words, fs, n, block_ms) in files.items():
            words.tofile(tmp / f"{name}.i8")
            self.handles[name] = self._open(self.ctx, tmp / f"{name}.i8", fs, n, block_ms)
        self.handles["host"] = self._open(None, tmp / "dev.i8", FS, N, 5)
        self.handles["chain"] = self._open(self.ctx, tmp / "dev.i8", FS, N, 5)
        path, g = str(tmp / "dev.i8").encode(), C.c_void_p()
        assert self.lib.gyp_ingest_open_resampled(self.ctx, path, _lib.GYP_FMT_I8, 2 * FS, 0, 5, 3, C.byref(g)) == 0 and g.value
        self.handles["resampled"] = g
        packing, g = np.zeros(1, dtype=_lib.PACKING), C.c_void_p()
        packing[0]["bits"], packing[0]["order"] = 2, _lib.GYP_PACK_MSB_FIRST
        assert self.lib.gyp_ingest_open_packed(self.ctx, path, _lib.ptr(packing), FS, 0, 0, 5, 3, C.byref(g)) == 0 and g.value
        self.handles["packed"] = g

    def _open(self, ctx, path, fs, n, block_ms):
        g = C.c_void_p()
        rc = self.lib.gyp_ingest_open(ctx, str(path).encode(), _lib.GYP_FMT_I8, fs, n, block_ms, 3, C.byref(g))
        assert rc == 0 and g.value, (path, rc)
        return g

    def close(self) -> None:
        for g in self.handles.values():
            self.lib.gyp_ingest_close(g)
        self.buf.free()
        self.eng.close()


def refused_calls(env: Env):
    """[(id, whose error text: the context's (True) or gyp_last_error(NULL)'s (False), the call)]."""
    lib, ctx, p = env.lib, env.ctx, env.p
    ptr = _lib.ptr
    dev, zeros, slow, wide, host = (env.handles[k] for k in ("dev", "zeros", "slow", "wide", "host"))
    rows = []

    def row(name, call, on_ctx=True):
        rows.append((name, on_ctx, call))

    # -------------------------------------------------------------------------------------------- gyp_iq_stats_dev
    def stats(c=ctx, iq=p, ns=1, stride=16, n_ms=1, n=16, out=p):
        return lambda: lib.gyp_iq_stats_dev(c, iq, ns, stride, n_ms, n, 0.0, out)
    row("stats: ctx NULL", stats(c=None), False)
    row("stats: iq NULL", stats(iq=None))
    row("stats: out NULL", stats(out=None))
    row("stats: n_streams 0", stats(ns=0))
    row("stats: n_ms 0", stats(n_ms=0))
    row("stats: samples_per_ms 0", stats(n=0))
    row("stats: stride", stats(ns=2, stride=31, n_ms=2))

    # -------------------------------------------------------------------------------------------- gyp_condition_iq_dev
    two_levels = np.concatenate([_level(), _level()])

    def cond(c=ctx, inp=p, out=p, ns=1, stride=16, n_samples=16, levels=_level()):
        return lambda: lib.gyp_condition_iq_dev(c, inp, out, ns, stride, n_samples, ptr(levels))
    row("condition: ctx NULL", cond(c=None), False)
    row("condition: in NULL", cond(inp=None))
    row("condition: out NULL", cond(out=None))
    row("condition: levels NULL", cond(levels=None))
    row("condition: n_streams 0", cond(ns=0))
    row("condition: n_samples < 0", cond(n_samples=-1))
    row("condition: stride", cond(ns=2, stride=15, levels=two_levels))
    row("condition: dc_re nan", cond(levels=_level(dc_re=NAN)))
    row("condition: dc_im inf", cond(levels=_level(dc_im=-INF)))
    row("condition: gain 0", cond(levels=_level(gain=0.0)))
    row("condition: gain inf", cond(levels=_level(gain=INF)))
    row("condition: reserved", cond(levels=_level(reserved=1)))
    row("condition: second level bad", cond(ns=2, stride=16, levels=np.concatenate([_level(), _level(gain=-1.0)])))

    # -------------------------------------------------------------------------------------------- gyp_iq_tones_dev
    def tones(c=ctx, iq=p, ns=1, stride=64, first=0, nb=1, block=64, fs=FS, freqs=_i64([1000]), n_freq=1, window=0, out=p):
        return lambda: lib.gyp_iq_tones_dev(c, iq, ns, stride, first, nb, block, fs, ptr(freqs), n_freq, window, out)
    row("tones: ctx NULL", tones(c=None), False)
    row("tones: iq NULL", tones(iq=None))
    row("tones: out NULL", tones(out=None))
    row("tones: freqs NULL", tones(freqs=None))
    row("tones: n_streams 0", tones(ns=0))
    row("tones: n_blocks 0", tones(nb=0))
    row("tones: block_samples 0", tones(block=0))
    row("tones: n_freq 0", tones(n_freq=0))
    row("tones: first < 0", tones(first=-1))
    row("tones: stride", tones(ns=2, stride=63))
    row("tones: fs 999", tones(fs=999, freqs=_i64([0])))
    row("tones: fs 2^31", tones(fs=2 ** 31))
    row("tones: window 2", tones(window=2))
    row("tones: window -1", tones(window=-1))
    row("tones: f = -fs", tones(freqs=_i64([-FS])))
    row("tones: f = fs", tones(freqs=_i64([FS])))
    row("tones: f = fs / 2", tones(freqs=_i64([FS // 2])))
    row("tones: second f = -fs / 2", tones(freqs=_i64([1000, -(FS // 2)]), n_freq=2))

    # -------------------------------------------------------------------------------------------- gyp_notch_iq_dev
    def notch(c=ctx, inp=p, out=p, ns=1, stride=N, first=0, n_ms=1, n=N, fs=FS, t=_tones([1000])):
        return lambda: lib.gyp_notch_iq_dev(c, inp, out, ns, stride, first, n_ms, n, fs, ptr(t))
    row("notch: ctx NULL", notch(c=None), False)
    row("notch: in NULL", notch(inp=None))
    row("notch: out NULL", notch(out=None))
    row("notch: tones NULL", notch(t=None))
    row("notch: n_streams 0", notch(ns=0))
    row("notch: n_ms < 0", notch(n_ms=-1))
    row("notch: samples_per_ms 0", notch(n=0))
    row("notch: first < 0", notch(first=-1))
    row("notch: stride", notch(ns=2, stride=N - 1, t=_tones([1000], n=2)))
    row("notch: fs 999", notch(fs=999, t=_tones([0])))
    row("notch: fs 2^31", notch(fs=2 ** 31))
    row("notch: reserved", notch(t=_tones([1000], reserved=1)))
    row("notch: count 9", notch(t=_tones([], count=9)))
    row("notch: count -1", notch(t=_tones([], count=-1)))
    row("notch: f = fs / 2", notch(t=_tones([FS // 2])))
    row("notch: f = -fs", notch(t=_tones([-FS])))
    row("notch: f = fs", notch(t=_tones([FS])))
    row("notch: 3999 Hz apart", notch(t=_tones([100_000, 103_999])))

    # -------------------------------------------------------------------------------------------- gyp_blank_iq_dev
    def blank(c=ctx, inp=p, out=p, ns=1, stride=N, n_ms=1, n=N, b=_blanker()):
        return lambda: lib.gyp_blank_iq_dev(c, inp, out, ns, stride, n_ms, n, ptr(b), None)
    row("blank: ctx NULL", blank(c=None), False)
    row("blank: in NULL", blank(inp=None))
    row("blank: out NULL", blank(out=None))
    row("blank: blankers NULL", blank(b=None))
    row("blank: n_streams 0", blank(ns=0))
    row("blank: n_ms < 0", blank(n_ms=-1))
    row("blank: samples_per_ms 0", blank(n=0))
    row("blank: samples_per_ms 65537", blank(n=65537, stride=65537))
    row("blank: stride", blank(ns=2, stride=N - 1, b=np.concatenate([_blanker(), _blanker()])))
    row("blank: centre inf", blank(b=_blanker(center_re=INF)))
    row("blank: centre nan", blank(b=_blanker(center_im=NAN)))
    row("blank: threshold 0", blank(b=_blanker(threshold=0.0)))
    row("blank: threshold inf", blank(b=_blanker(threshold=INF)))
    row("blank: guard -1", blank(b=_blanker(guard=-1)))
    row("blank: guard 65", blank(b=_blanker(guard=65)))

    # -------------------------------------------------------------------------------------------- gyp_iq_power_hist_dev
    def hist(c=ctx, iq=p, ns=1, stride=N, n_samples=N, centres=None, out=p):
        return lambda: lib.gyp_iq_power_hist_dev(c, iq, ns, stride, n_samples, ptr(centres), out)
    row("hist: ctx NULL", hist(c=None), False)
    row("hist: iq NULL", hist(iq=None))
    row("hist: hist NULL", hist(out=None))
    row("hist: n_streams 0", hist(ns=0))
    row("hist: n_samples 0", hist(n_samples=0))
    row("hist: stride", hist(ns=2, stride=N - 1))
    row("hist: centre inf", hist(centres=np.array([INF, 0.0], dtype=np.float32)))
    row("hist: second centre nan", hist(ns=2, centres=np.array([0.0, 0.0, 0.0, NAN], dtype=np.float32)))

    # -------------------------------------------------------------------------------------------- gyp_excise_iq_dev
    def excise(c=ctx, inp=p, out=p, ns=1, stride=N, n_ms=1, n=N, e=_excisor()):
        return lambda: lib.gyp_excise_iq_dev(c, inp, out, ns, stride, n_ms, n, ptr(e), None, None)
    row("excise: ctx NULL", excise(c=None), False)
    row("excise: in NULL", excise(inp=None))
    row("excise: out NULL", excise(out=None))
    row("excise: excisors NULL", excise(e=None))
    row("excise: n_streams 0", excise(ns=0))
    row("excise: n_ms < 0", excise(n_ms=-1))
    row("excise: samples_per_ms 0", excise(n=0))
    row("excise: samples_per_ms 65537", excise(n=65537, stride=65537))
    row("excise: stride", excise(ns=2, stride=N - 1, e=np.concatenate([_excisor(), _excisor()])))
    row("excise: threshold 0", excise(e=_excisor(threshold=0.0)))
    row("excise: threshold inf", excise(e=_excisor(threshold=INF)))
    row("excise: threshold nan", excise(e=_excisor(threshold=NAN)))
    row("excise: guard -1", excise(e=_excisor(guard=-1)))
    row("excise: guard 9", excise(e=_excisor(guard=9)))
    row("excise: reserved[0]", excise(e=_excisor(reserved=(1, 0))))
    row("excise: reserved[1]", excise(e=_excisor(reserved=(0, 1))))
    row("excise: second excisor bad", excise(ns=2, e=np.concatenate([_excisor(), _excisor(guard=9)])))

    # -------------------------------------------------------------------------------------------- gyp_iq_spectrum_hist_dev
    def spectrum(c=ctx, iq=p, ns=1, stride=N, n_ms=1, n=N, out=p):
        return lambda: lib.gyp_iq_spectrum_hist_dev(c, iq, ns, stride, n_ms, n, out)
    row("spectrum_hist: ctx NULL", spectrum(c=None), False)
    row("spectrum_hist: iq NULL", spectrum(iq=None))
    row("spectrum_hist: hist NULL", spectrum(out=None))
    row("spectrum_hist: n_streams 0", spectrum(ns=0))
    row("spectrum_hist: n_ms 0", spectrum(n_ms=0))
    row("spectrum_hist: samples_per_ms 255", spectrum(n=255, stride=255))
    row("spectrum_hist: samples_per_ms 65537", spectrum(n=65537, stride=65537))
    row("spectrum_hist: stride", spectrum(ns=2, stride=N - 1))

    # -------------------------------------------------------------------------------------------- gyp_track_quality_dev
    def quality(c=ctx, recs=p, nc=1, stride=20, n_ms=20, window=20, offsets=None, out=p):
        return lambda: lib.gyp_track_quality_dev(c, recs, nc, stride, n_ms, window, ptr(offsets), out)
    row("quality: ctx NULL", quality(c=None), False)
    row("quality: recs NULL", quality(recs=None))
    row("quality: out NULL", quality(out=None))
    row("quality: n_chan 0", quality(nc=0))
    row("quality: n_ms 0", quality(n_ms=0))
    row("quality: window_ms 0", quality(window=0))
    row("quality: stride", quality(nc=2, stride=19))
    row("quality: bit offset -2", quality(offsets=np.array([-2], dtype=np.int32)))
    row("quality: second bit offset 20", quality(nc=2, offsets=np.array([0, 20], dtype=np.int32)))

    # -------------------------------------------------------------------------------------------- the ingest handle
    enabled, count = C.c_int32(), C.c_int32()
    level_out, blanker_out, excisor_out = _level(), _blanker(), _excisor()
    freqs8, counts = np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int32)

    def both(name, call):
        """The pair that opens an entry point: no handle, and a handle opened without a context."""
        row(f"{name}: handle NULL", lambda: call(None), False)
        row(f"{name}: no context", lambda: call(host), False)

    both("set_level", lambda g: lib.gyp_ingest_set_level(g, ptr(_level())))
    row("set_level: gain 0", lambda: lib.gyp_ingest_set_level(dev, ptr(_level(gain=0.0))))
    row("set_level: dc nan", lambda: lib.gyp_ingest_set_level(dev, ptr(_level(dc_re=NAN))))
    row("set_level: reserved", lambda: lib.gyp_ingest_set_level(dev, ptr(_level(reserved=1))))
    both("get_level", lambda g: lib.gyp_ingest_get_level(g, ptr(level_out), C.byref(enabled)))

    def calibrate(g=dev, first=0, n_ms=5, target=0.05):
        return lambda: lib.gyp_ingest_calibrate(g, first, n_ms, 1, target, 0.0, ptr(level_out), None)
    both("calibrate", lambda g: calibrate(g=g)())
    row("calibrate: n_ms 0", calibrate(n_ms=0))
    row("calibrate: n_ms 10001", calibrate(n_ms=10001))
    row("calibrate: first < 0", calibrate(first=-1))
    row("calibrate: past the end", calibrate(first=36))
    row("calibrate: target_rms 0", calibrate(target=0.0))
    row("calibrate: target_rms inf", calibrate(target=INF))
    row("calibrate: target_rms nan", calibrate(target=NAN))
    row("calibrate: a constant recording", calibrate(g=zeros))

    both("set_notches", lambda g: lib.gyp_ingest_set_notches(g, ptr(_i64([1000])), 1))
    row("set_notches: count 9", lambda: lib.gyp_ingest_set_notches(dev, ptr(_i64(range(0, 90_000, 10_000))), 9))
    row("set_notches: f = fs / 2", lambda: lib.gyp_ingest_set_notches(dev, ptr(_i64([FS // 2])), 1))
    row("set_notches: 3999 Hz apart", lambda: lib.gyp_ingest_set_notches(dev, ptr(_i64([100_000, 103_999])), 2))
    both("get_notches", lambda g: lib.gyp_ingest_get_notches(g, ptr(freqs8), C.byref(count)))

    def find_tones(g=dev, first=0, n_ms=5, threshold=8.0, max_tones=4, n_out=count):
        return lambda: lib.gyp_ingest_find_tones(g, first, n_ms, threshold, max_tones, 0, ptr(freqs8), None, C.byref(n_out) if n_out is not None else None)
    both("find_tones", lambda g: find_tones(g=g)())
    row("find_tones: n_out NULL", find_tones(n_out=None))
    row("find_tones: n_ms 0", find_tones(n_ms=0))
    row("find_tones: n_ms 1001", find_tones(n_ms=1001))
    row("find_tones: first < 0", find_tones(first=-1))
    row("find_tones: past the end", find_tones(first=36))
    row("find_tones: threshold 0", find_tones(threshold=0.0))
    row("find_tones: threshold inf", find_tones(threshold=INF))
    row("find_tones: max_tones 0", find_tones(max_tones=0))
    row("find_tones: max_tones 9", find_tones(max_tones=9))
    row("find_tones: fewer than 1024 samples", find_tones(g=slow, n_ms=1000))

    both("set_blanker", lambda g: lib.gyp_ingest_set_blanker(g, ptr(_blanker())))
    row("set_blanker: centre nan", lambda: lib.gyp_ingest_set_blanker(dev, ptr(_blanker(center_re=NAN))))
    row("set_blanker: threshold 0", lambda: lib.gyp_ingest_set_blanker(dev, ptr(_blanker(threshold=0.0))))
    row("set_blanker: guard 65", lambda: lib.gyp_ingest_set_blanker(dev, ptr(_blanker(guard=65))))
    row("set_blanker: 65537 samples per ms", lambda: lib.gyp_ingest_set_blanker(wide, ptr(_blanker())))
    both("get_blanker", lambda g: lib.gyp_ingest_get_blanker(g, ptr(blanker_out), C.byref(enabled)))

    def find_pulses(g=dev, first=0, n_ms=5, threshold=16.0, guard=4):
        return lambda: lib.gyp_ingest_find_pulses(g, first, n_ms, 1, threshold, guard, 0, ptr(blanker_out), None)
    both("find_pulses", lambda g: find_pulses(g=g)())
    row("find_pulses: n_ms 0", find_pulses(n_ms=0))
    row("find_pulses: n_ms 1001", find_pulses(n_ms=1001))
    row("find_pulses: first < 0", find_pulses(first=-1))
    row("find_pulses: past the end", find_pulses(first=36))
    row("find_pulses: threshold 0", find_pulses(threshold=0.0))
    row("find_pulses: threshold nan", find_pulses(threshold=NAN))
    row("find_pulses: guard -1", find_pulses(guard=-1))
    row("find_pulses: guard 65", find_pulses(guard=65))
    row("find_pulses: 65537 samples per ms", find_pulses(g=wide, n_ms=1))

    both("last_blanked", lambda g: lib.gyp_ingest_last_blanked(g, ptr(counts), 8, C.byref(count)))
    row("last_blanked: n_ms_out NULL", lambda: lib.gyp_ingest_last_blanked(dev, ptr(counts), 8, None))
    row("last_blanked: cap < 0", lambda: lib.gyp_ingest_last_blanked(dev, ptr(counts), -1, C.byref(count)))
    row("last_blanked: cap without counts_out", lambda: lib.gyp_ingest_last_blanked(dev, None, 8, C.byref(count)))

    both("set_excisor", lambda g: lib.gyp_ingest_set_excisor(g, ptr(_excisor())))
    row("set_excisor: threshold 0", lambda: lib.gyp_ingest_set_excisor(dev, ptr(_excisor(threshold=0.0))))
    row("set_excisor: threshold inf", lambda: lib.gyp_ingest_set_excisor(dev, ptr(_excisor(threshold=INF))))
    row("set_excisor: guard 9", lambda: lib.gyp_ingest_set_excisor(dev, ptr(_excisor(guard=9))))
    row("set_excisor: reserved", lambda: lib.gyp_ingest_set_excisor(dev, ptr(_excisor(reserved=(0, 1)))))
    row("set_excisor: 65537 samples per ms", lambda: lib.gyp_ingest_set_excisor(wide, ptr(_excisor())))
    both("get_excisor", lambda g: lib.gyp_ingest_get_excisor(g, ptr(excisor_out), C.byref(enabled)))

    def find_excisor(g=dev, first=0, n_ms=5, threshold=16.0, guard=1):
        return lambda: lib.gyp_ingest_find_excisor(g, first, n_ms, threshold, guard, 0, ptr(excisor_out), None)
    both("find_excisor", lambda g: find_excisor(g=g)())
    row("find_excisor: n_ms 0", find_excisor(n_ms=0))
    row("find_excisor: n_ms 1001", find_excisor(n_ms=1001))
    row("find_excisor: first < 0", find_excisor(first=-1))
    row("find_excisor: past the end", find_excisor(first=36))
    row("find_excisor: threshold 0", find_excisor(threshold=0.0))
    row("find_excisor: threshold nan", find_excisor(threshold=NAN))
    row("find_excisor: guard -1", find_excisor(guard=-1))
    row("find_excisor: guard 9", find_excisor(guard=9))
    row("find_excisor: 65537 samples per ms", find_excisor(g=wide, n_ms=1))
    row("find_excisor: fewer than 256 samples per ms", find_excisor(g=slow))

    both("last_excised", lambda g: lib.gyp_ingest_last_excised(g, ptr(counts), 8, C.byref(count)))
    row("last_excised: n_ms_out NULL", lambda: lib.gyp_ingest_last_excised(dev, ptr(counts), 8, None))
    row("last_excised: cap < 0", lambda: lib.gyp_ingest_last_excised(dev, ptr(counts), -1, C.byref(count)))
    row("last_excised: cap without counts_out", lambda: lib.gyp_ingest_last_excised(dev, None, 8, C.byref(count)))

    # gyp_ingest_next_host: a stage of `chain` is switched on for the row alone and off again behind it (a call that succeeds
    # leaves the error text as it is)
    chain, resampled, packed = (env.handles[k] for k in ("chain", "resampled", "packed"))
    raw, first, n_ms = C.c_void_p(), C.c_int64(), C.c_int32()

    def next_host(g=chain, raw_out=raw, first_out=first, n_out=n_ms):
        byref = lambda x: C.byref(x) if x is not None else None   # noqa: E731
        return lambda: lib.gyp_ingest_next_host(g, byref(raw_out), byref(first_out), byref(n_out))
    stages = {"level": (lambda: lib.gyp_ingest_set_level(chain, ptr(_level(gain=2.0))), lambda: lib.gyp_ingest_set_level(chain, None)),
              "notches": (lambda: lib.gyp_ingest_set_notches(chain, ptr(_i64([100_000])), 1), lambda: lib.gyp_ingest_set_notches(chain, None, 0)),
              "blanker": (lambda: lib.gyp_ingest_set_blanker(chain, ptr(_blanker())), lambda: lib.gyp_ingest_set_blanker(chain, None)),
              "excisor": (lambda: lib.gyp_ingest_set_excisor(chain, ptr(_excisor())), lambda: lib.gyp_ingest_set_excisor(chain, None))}

    def with_stages(names, call=next_host()):
        def run():
            for k in names:
                assert stages[k][0]() == 0
            rc = call()
            for k in names:
                assert stages[k][1]() == 0
            return rc
        return run

    def in_flight():
        iq = C.c_void_p()
        assert lib.gyp_ingest_next_dev(chain, C.byref(iq), C.byref(first), C.byref(n_ms)) == 0 and n_ms.value == 5
        rc = next_host()()
        assert lib.gyp_ingest_seek(chain, 0) == 0
        return rc
    row("next_host: handle NULL", next_host(g=None), False)
    row("next_host: raw_out NULL", next_host(raw_out=None))
    row("next_host: first_ms_out NULL", next_host(first_out=None))
    row("next_host: n_ms_out NULL", next_host(n_out=None))
    row("next_host: a resampled handle", next_host(g=resampled))
    row("next_host: a packed handle", next_host(g=packed))
    row("next_host: a level is on", with_stages(["level"]))
    row("next_host: notches are on", with_stages(["notches"]))
    row("next_host: a blanker is on", with_stages(["blanker"]))
    row("next_host: an excisor is on", with_stages(["excisor"]))
    row("next_host: excisor and blanker on", with_stages(["excisor", "blanker"]))
    row("next_host: excisor, blanker and notches on", with_stages(["excisor", "blanker", "notches"]))
    row("next_host: all four on", with_stages(["excisor", "blanker", "notches", "level"]))
    row("next_host: device blocks in flight", in_flight)
    return rows


NULL_SENTINEL = "gyp_create: out is NULL"


def run_table(env: Env):
    """{id: [code, text]} of every row, each behind the sentinels."""
    lib, got = env.lib, {}
    for name, on_ctx, call in refused_calls(env):
        assert lib.gyp_debug_set(env.ctx, b"no_such_switch", 0.0) != 0 and lib.gyp_create(0, None) != 0
        assert lib.gyp_last_error(None).decode() == NULL_SENTINEL
        before = lib.gyp_last_error(env.ctx).decode()
        rc = call()
        text = lib.gyp_last_error(env.ctx if on_ctx else None).decode()
        assert name not in got, name
        got[name] = [int(rc), text, before]
    return got


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    e = Env(tmp_path_factory.mktemp("refusals"))
    yield e
    e.close()


def test_every_refusal_keeps_its_code_and_its_text(env):
    want = json.loads(GOLDEN.read_text())
    got = run_table(env)
    assert list(got) == list(want)                       # the same rows in the same order
    for name, (code, text, before) in got.items():
        assert [code, text] == want[name], name
        assert code < 0 and text and text != before and text != NULL_SENTINEL, name      # refused, with a text of its own
    # a refused call changes nothing: the handle has no level, notches, blanker or excisor, and serves its first block
    lib, dev = env.lib, env.handles["dev"]
    enabled, count = C.c_int32(-1), C.c_int32(-1)
    assert lib.gyp_ingest_get_level(dev, None, C.byref(enabled)) == 0 and enabled.value == 0
    assert lib.gyp_ingest_get_blanker(dev, None, C.byref(enabled)) == 0 and enabled.value == 0
    assert lib.gyp_ingest_get_excisor(dev, None, C.byref(enabled)) == 0 and enabled.value == 0
    assert lib.gyp_ingest_get_notches(dev, None, C.byref(count)) == 0 and count.value == 0
    iq, first, n_ms = C.c_void_p(), C.c_int64(-1), C.c_int32(-1)
    assert lib.gyp_ingest_next_dev(dev, C.byref(iq), C.byref(first), C.byref(n_ms)) == 0 and (first.value, n_ms.value) == (0, 5)
    env.eng.sync()
