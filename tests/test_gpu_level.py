"""Signal conditioning on the device (gyp_iq_stats_dev, gyp_condition_iq_dev, gyp_ingest_set_level / _calibrate): the statistics
against numpy's exact integer sums and math.fsum, bit-identical for every call shape, window, alignment and grid size; the condition
kernel against numpy's float32 (x - dc) * g bit for bit; a level on every kind of ingest handle; the calibration against the Python
model of tests/level_model.py; and an offset-binary recording that cannot be acquired as it is, acquired."""
from __future__ import annotations

import math

import numpy as np
import pytest

import level_model as model
from gypsum_amd import _lib
from gypsum_amd import packing as pk
from gypsum_amd.antenna_sample_provider import AntennaSampleProviderResampled
from gypsum_amd.engine import GypsumEngine
from gypsum_amd.ingest import IqFileIngest
from gypsum_amd.level import STATS_DTYPE, IqLevel, default_target_rms
from oracle import gypsum_oracle as orc

pytestmark = pytest.mark.gpu

BAD = _lib.GYP_E_BAD_ARG
G = float(np.float32(0.01))


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(fs: int) -> GypsumEngine:
        if fs not in made:
            eng = GypsumEngine(0)
            eng.set_stream_format(fs, fs // 1000)
            made[fs] = eng
        return made[fs]

    yield get
    for eng in made.values():
        eng.close()


def _same(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _stats(eng, flat: np.ndarray, offset: int, n_streams: int, stride: int, n_ms: int, n: int, clip: float = 0.0) -> np.ndarray:
    """gyp_iq_stats_dev on complex64 `flat` uploaded as it is, the first stream starting `offset` samples into the buffer."""
    assert offset + (n_streams - 1) * stride + n_ms * n <= flat.size     # the kernel reads nothing else
    d_iq = eng.alloc(flat.nbytes).upload(flat)
    d_out = eng.alloc(n_streams * n_ms * STATS_DTYPE.itemsize)
    eng.iq_stats_dev(d_iq.ptr.value + 8 * offset, n_streams, stride, n_ms, n, clip, d_out.ptr.value)
    out = d_out.download(STATS_DTYPE, n_streams * n_ms).reshape(n_streams, n_ms)
    d_iq.free()
    d_out.free()
    return out


def _int_samples(rng, count: int, bound: int) -> np.ndarray:
    w = rng.integers(-bound, bound + 1, 2 * count)
    x = np.empty(count, dtype=np.complex64)
    x.real, x.imag = w[0::2], w[1::2]
    return x


def _exact_stats(x: np.ndarray, n: int, clip: float) -> np.ndarray:
    words = np.empty(2 * x.size, dtype=np.int64)
    words[0::2], words[1::2] = x.real, x.imag
    return model.stats_of_words(words, n, clip)


# ---------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("n", [7, 1000, 1023, 2046, 8184])
def test_stats_of_integer_samples_are_exact(engines, n):
    """Fewer samples than threads, a length that is no format, odd N (every other row 8-byte aligned only) and the two common
    formats; 2 streams at stride n_ms N + 3 from a base one sample into the buffer."""
    eng = engines(2_046_000)
    rng = np.random.default_rng(n)
    for n_ms in (1, 3):
        stride = n_ms * n + 3
        for bound, clip in ((32767, 0.0), (127, 127.0)):
            flat = _int_samples(rng, 1 + 2 * stride, bound)
            got = _stats(eng, flat, 1, 2, stride, n_ms, n, clip)
            for s in range(2):
                want = _exact_stats(flat[1 + s * stride:1 + s * stride + n_ms * n], n, clip)
                for f in STATS_DTYPE.names:
                    assert np.array_equal(got[s][f], want[f]), (n, n_ms, bound, s, f, got[s][f], want[f])
            if clip:
                assert got["n_clip"].sum() > 0 or n == 7
            else:
                assert not got["n_clip"].any()


def test_stats_of_more_items_than_the_grid_holds_and_any_grid_size(engines):
    """2 x 300 ms at N = 1023 in one call: 600 items over a persistent grid of at most 512 workgroups; the same bits at 1 and 8
    workgroups per CU."""
    eng = engines(2_046_000)
    n, n_ms = 1023, 300
    flat = _int_samples(np.random.default_rng(600), 2 * n_ms * n, 32767)
    got = _stats(eng, flat, 0, 2, n_ms * n, n_ms, n, 30000.0)
    want = _exact_stats(flat, n, 30000.0).reshape(2, n_ms)
    for f in STATS_DTYPE.names:
        assert np.array_equal(got[f], want[f]), f
    try:
        for per_cu in (1, 8):
            eng.debug_set("widen_wg_per_cu", per_cu)
            assert _same(_stats(eng, flat, 0, 2, n_ms * n, n_ms, n, 30000.0), got), per_cu
    finally:
        eng.debug_set("widen_wg_per_cu", 2)


def test_stats_of_float_samples_are_accurate_and_the_same_for_every_call_shape(engines):
    eng = engines(2_046_000)
    n, n_ms = 49104, 3
    rng = np.random.default_rng(49104)
    flat = (rng.standard_normal(2 * n_ms * n) * 3.0 + 0.25 + 1j * (rng.standard_normal(2 * n_ms * n) * 0.5 - 1.0)).astype(np.complex64)
    got = _stats(eng, flat, 0, 2, n_ms * n, n_ms, n, 6.0)
    u = n * 2.0 ** -53     # the worst case of N float64 additions, relative to the sum of the terms' magnitudes
    for s in range(2):
        for m in range(n_ms):
            x = flat[(s * n_ms + m) * n:(s * n_ms + m + 1) * n]
            re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
            sq = np.concatenate([re * re, im * im])          # float32 squared is exact in float64
            for f, terms in (("sum_re", re), ("sum_im", im), ("sum_sq", sq)):
                ref, mag = math.fsum(terms), math.fsum(np.abs(terms))
                err = abs(float(got[s, m][f]) - ref)
                print(f"{f} stream {s} ms {m}: |error| {err:.3e}, bound {u * mag:.3e}")
                assert err <= u * mag, (f, s, m, err, u * mag)
            assert got[s, m]["max_abs"] == max(np.abs(x.real).max(), np.abs(x.imag).max())
            assert got[s, m]["n_clip"] == (np.abs(x.real) >= 6.0).sum() + (np.abs(x.imag) >= 6.0).sum()
    assert _same(_stats(eng, flat, 0, 2, n_ms * n, n_ms, n, 6.0), got)                       # two runs
    one = _stats(eng, flat, (1 * n_ms + 2) * n, 1, 0, 1, n, 6.0)                              # (stream 1, ms 2) alone, in place
    assert _same(one[0, 0], got[1, 2])
    moved = np.concatenate([np.zeros(1, np.complex64), flat[(1 * n_ms + 2) * n:(1 * n_ms + 3) * n]])
    assert _same(_stats(eng, moved, 1, 1, 0, 1, n, 6.0)[0, 0], got[1, 2])                     # the same samples, 8-byte aligned only
    assert _same(_stats(eng, flat, n_ms * n, 1, 0, n_ms, n, 6.0)[0], got[1])                  # stream 1 alone


def test_stats_arguments_are_checked(engines):
    eng = engines(2_046_000)
    d = eng.alloc(4096)
    cases = {"iq NULL": (0, 1, 16, 1, 16, d.ptr.value), "out NULL": (d.ptr.value, 1, 16, 1, 16, 0), "n_streams 0": (d.ptr.value, 0, 16, 1, 16, d.ptr.value),
             "n_ms 0": (d.ptr.value, 1, 16, 0, 16, d.ptr.value), "N 0": (d.ptr.value, 1, 16, 1, 0, d.ptr.value),
             "stride": (d.ptr.value, 2, 31, 2, 16, d.ptr.value)}
    for what, (iq, ns, stride, n_ms, n, out) in cases.items():
        with pytest.raises(_lib.GypsumHipError, match="gyp_iq_stats_dev") as e:
            eng.iq_stats_dev(iq, ns, stride, n_ms, n, 0.0, out)
        assert e.value.code == BAD, what
    d.free()


# ---------------------------------------------------------------------------------------------------- condition
def _condition(eng, flat, offset, n_streams, stride, n_samples, levels, in_place):
    """(output buffer, input buffer) after gyp_condition_iq_dev, whole buffers downloaded; out of place the output starts as NaN."""
    assert offset + (n_streams - 1) * stride + n_samples <= flat.size
    d_in = eng.alloc(flat.nbytes).upload(flat)
    d_out = d_in if in_place else eng.alloc(flat.nbytes).upload(np.full(flat.size, np.nan + 0j, dtype=np.complex64))
    eng.condition_iq_dev(d_in.ptr.value + 8 * offset, d_out.ptr.value + 8 * offset, n_streams, stride, n_samples, levels)
    out, src = d_out.download(np.complex64, flat.size), d_in.download(np.complex64, flat.size)
    d_in.free()
    if not in_place:
        d_out.free()
    return out, src


def _numpy_condition(x: np.ndarray, level: IqLevel) -> np.ndarray:
    f = x.view(np.float32).reshape(-1, 2)
    dc = np.array([level.dc_re, level.dc_im], dtype=np.float32)
    y = (f - dc) * np.float32(level.gain)
    assert y.dtype == np.float32
    return y.reshape(-1).view(np.complex64)


@pytest.mark.parametrize("offset,n_streams,pad,n_samples", [(1, 2, 3, 3 * 1023 + 5), (0, 2, 4, 3 * 1023 + 5), (0, 1, 0, 3 * 1023 + 4), (0, 2, 1, 1)])
def test_condition_equals_numpy_float32_bit_for_bit(engines, offset, n_streams, pad, n_samples):
    """An 8-byte-aligned base with an odd stride (8-byte accesses), 16-byte-aligned rows, an odd count behind 16-byte accesses."""
    eng = engines(2_046_000)
    rng = np.random.default_rng(n_samples + pad)
    stride = n_samples + pad
    flat = (rng.standard_normal(offset + n_streams * stride) * 40 + 128 + 1j * (rng.standard_normal(offset + n_streams * stride) * 40 + 127)).astype(np.complex64)
    levels = [IqLevel(128.0, 127.5, G), IqLevel(-3.25, 0.1, 7.3)][:n_streams]
    for in_place in (False, True):
        out, src = _condition(eng, flat, offset, n_streams, stride, n_samples, levels, in_place)
        touched = np.zeros(flat.size, dtype=bool)
        for s, level in enumerate(levels):
            a = offset + s * stride
            assert _same(out[a:a + n_samples], _numpy_condition(flat[a:a + n_samples], level)), (in_place, s)
            touched[a:a + n_samples] = True
        if in_place:
            assert _same(out[~touched], flat[~touched])
        else:
            assert np.isnan(out[~touched].real).all() and _same(src, flat)
        unit, _ = _condition(eng, flat, offset, n_streams, stride, n_samples, [IqLevel()] * n_streams, in_place)
        assert _same(unit[touched], flat[touched])           # {0, 0, 1} returns the input bits


def test_bad_levels_are_refused(engines):
    eng = engines(2_046_000)
    d = eng.alloc(4096)
    for level in (IqLevel(0, 0, 0.0), IqLevel(0, 0, -1.0), IqLevel(0, 0, np.inf), IqLevel(0, 0, np.nan), IqLevel(np.nan, 0, 1.0),
                  IqLevel(0, -np.inf, 1.0)):
        with pytest.raises(_lib.GypsumHipError, match="gyp_condition_iq_dev") as e:
            eng.condition_iq_dev(d.ptr.value, d.ptr.value, 1, 16, 16, level)
        assert e.value.code == BAD, level
    rec = IqLevel().record()
    rec["reserved"] = 1
    with pytest.raises(_lib.GypsumHipError, match="reserved"):
        eng.condition_iq_dev(d.ptr.value, d.ptr.value, 1, 16, 16, rec)
    with pytest.raises(_lib.GypsumHipError, match="gyp_condition_iq_dev"):
        eng.condition_iq_dev(d.ptr.value, d.ptr.value, 2, 15, 16, [IqLevel(), IqLevel()])
    with pytest.raises(_lib.GypsumHipError, match="gyp_condition_iq_dev"):
        eng.condition_iq_dev(0, d.ptr.value, 1, 16, 16, IqLevel())
    d.free()


# ---------------------------------------------------------------------------------------------------- ingest
def _drain(eng, ing):
    """Every device block from the handle's position on, downloaded: (first ms of each block, concatenated samples)."""
    got, firsts = [], []
    while (blk := ing.next_device_block()) is not None:
        f, count, dev = blk
        buf = np.empty(count * ing.n, dtype=np.complex64)
        eng._check(eng.lib.gyp_memcpy_d2h(eng.ctx, _lib.ptr(buf), _lib.C.c_void_p(dev), buf.nbytes))
        got.append(buf)
        firsts.append(f)
    return firsts, (np.concatenate(got) if got else np.empty(0, np.complex64))


def _next(eng, ing):
    f, count, dev = ing.next_device_block()
    buf = np.empty(count * ing.n, dtype=np.complex64)
    eng._check(eng.lib.gyp_memcpy_d2h(eng.ctx, _lib.ptr(buf), _lib.C.c_void_p(dev), buf.nbytes))
    return f, buf


@pytest.fixture(scope="module")
def twin_files(tmp_path_factory):
    """A 40-ms recording at 2.046 Msps as uint8 words w8 + 128 and as its int8 twin w8 (one sample more than 40 ms: total_ms = 40)."""
    d = tmp_path_factory.mktemp("level")
    rng = np.random.default_rng(40)
    w8 = np.clip(np.rint(rng.normal(0.0, 20.0, 2 * (40 * 2046 + 1))), -127, 127).astype(np.int8)
    u8 = (w8.astype(np.int16) + 128).astype(np.uint8)
    w8.tofile(d / "twin.i8")
    u8.tofile(d / "rec.u8")
    return d / "rec.u8", d / "twin.i8", u8, w8


def _as_complex(words: np.ndarray) -> np.ndarray:
    x = np.empty(words.size // 2, dtype=np.complex64)
    x.real, x.imag = words[0::2], words[1::2]
    return x


@pytest.mark.parametrize("block_ms", [1, 7, 250])
def test_a_level_on_the_uint8_handle_equals_the_scaled_int8_twin(engines, twin_files, block_ms):
    """(float(u8) - 128) * g and float(w8) * g are the same single rounding: blocks, a seek to an odd millisecond and EOF."""
    eng = engines(2_046_000)
    rec, twin, u8, w8 = twin_files
    a = IqFileIngest(rec, 2_046_000, np.uint8, block_ms=block_ms, depth=3, engine=eng)
    b = IqFileIngest(twin, 2_046_000, np.int8, block_ms=block_ms, depth=3, engine=eng)
    try:
        assert a.total_ms == b.total_ms == 40 and a.level is None
        a.set_level(IqLevel(128.0, 128.0, G))
        assert a.level == IqLevel(128.0, 128.0, G)
        b.set_scale(G)
        for at in (None, 11, 39):
            if at is not None:
                a.seek(at)
                b.seek(at)
            fa, xa = _drain(eng, a)
            fb, xb = _drain(eng, b)
            assert fa == fb and fa[0] == (at or 0) and xa.size == (40 - (at or 0)) * 2046
            assert _same(xa, xb), (block_ms, at)
        assert _same(xb.view(np.float32), w8[2 * 39 * 2046:2 * 40 * 2046].astype(np.float32) * np.float32(G))
        a.set_level(None)                                     # the raw values again, from where the handle stood (EOF) and after a seek
        assert a.level is None and a.next_device_block() is None
        a.seek(0)
        _, raw = _drain(eng, a)
        assert _same(raw, _as_complex(u8[:2 * 40 * 2046]))
    finally:
        a.close()
        b.close()


def test_a_level_set_between_two_blocks_applies_from_the_next_block(engines, twin_files):
    eng = engines(2_046_000)
    rec, _, u8, _ = twin_files
    ing = IqFileIngest(rec, 2_046_000, np.uint8, block_ms=7, depth=3, engine=eng)
    try:
        level = IqLevel(127.0, 129.0, 0.125)
        x = _as_complex(u8[:2 * 40 * 2046])
        f0, b0 = _next(eng, ing)                      # block 1 is already uploaded ahead, without a level
        ing.set_level(level)
        f1, b1 = _next(eng, ing)
        ing.set_level(None)
        f2, b2 = _next(eng, ing)
        assert (f0, f1, f2) == (0, 7, 14)
        assert _same(b0, x[:7 * 2046]) and _same(b1, _numpy_condition(x[7 * 2046:14 * 2046], level)) and _same(b2, x[14 * 2046:21 * 2046])
        ing.set_level(level)
        with pytest.raises(_lib.GypsumHipError, match="gyp_ingest_next_host") as e:      # host blocks are raw words
            ing.next_host_block()
        assert e.value.code == BAD
        with pytest.raises(_lib.GypsumHipError, match="gyp_ingest_set_level"):
            ing.set_level(IqLevel(0.0, 0.0, 0.0))
        assert ing.level == level
    finally:
        ing.close()


def _producer(kind: str, tmp_path, engines):
    """(engine, arguments of IqFileIngest) of one small handle per producer of a device block."""
    rng = np.random.default_rng(len(kind))
    path = tmp_path / f"{kind}.bin"
    if kind == "float32":          # native rate: the path with no kernel
        (rng.standard_normal(2 * (20 * 2046 + 1)) * 0.1 + 0.02).astype(np.float32).tofile(path)
        return engines(2_046_000), dict(path=path, samples_per_second=2_046_000, sample_component_data_type=np.float32)
    if kind == "resampled":        # int16, 2.048 -> 2.046 Msps
        np.rint(rng.normal(300.0, 2000.0, 2 * (20 * 2048 + 1))).astype(np.int16).tofile(path)
        return engines(2_046_000), dict(path=path, samples_per_second=2_046_000, sample_component_data_type=np.int16, resample_from_hz=2_048_000)
    if kind == "ddc":              # real int8, 16.368 Msps at IF 4.092 MHz -> 4.092 Msps
        np.clip(np.rint(rng.normal(5.0, 30.0, 20 * 16368 + 1)), -127, 127).astype(np.int8).tofile(path)
        return engines(4_092_000), dict(path=path, samples_per_second=4_092_000, sample_component_data_type=np.int8,
                                        resample_from_hz=16_368_000, if_hz=4_092_000)
    p = pk.sign_magnitude(2)       # packed 2-bit I,Q at the native rate
    path.write_bytes(pk.pack(rng.integers(0, 4, 2 * (20 * 2046 + 4)), p))
    return engines(2_046_000), dict(path=path, samples_per_second=2_046_000, packing=p)


@pytest.mark.parametrize("kind", ["float32", "resampled", "ddc", "packed"])
def test_a_level_conditions_the_blocks_of_every_producer(engines, tmp_path, kind):
    eng, kw = _producer(kind, tmp_path, engines)
    ing = IqFileIngest(block_ms=7, depth=3, engine=eng, **kw)
    try:
        level = IqLevel(0.75, -1.5, 0.3)
        firsts, plain = _drain(eng, ing)
        assert ing.total_ms == 20 and firsts == [0, 7, 14] and plain.size == 20 * ing.n and np.abs(plain).max() > 0
        ing.set_level(level)
        ing.seek(0)
        firsts2, got = _drain(eng, ing)
        assert firsts2 == firsts
        assert _same(got, eng.condition_iq(plain, level)) and _same(got, _numpy_condition(plain, level))
    finally:
        ing.close()


def test_calibrate_equals_the_model_on_the_files_words_whatever_the_blocks(engines, twin_files):
    eng = engines(2_046_000)
    rec, _, u8, _ = twin_files
    n, target = 2046, 0.05
    words = u8[2 * 5 * n:2 * 25 * n]
    want_level, want_measured = model.level_from_stats(model.stats_of_words(words, n, 170.0), n, True, target)
    x = _as_complex(u8[:2 * 40 * n])
    for block_ms in (1, 7, 20):
        ing = IqFileIngest(rec, 2_046_000, np.uint8, block_ms=block_ms, depth=3, engine=eng)
        try:
            f0, _ = _next(eng, ing)
            level, measured = ing.calibrate(first_ms=5, n_ms=20, target_rms=target, clip_level=170.0)
            got = np.array([level.dc_re, level.dc_im, level.gain], dtype=np.float32)
            assert _same(got, want_level), (block_ms, got, want_level)
            assert _same(np.array([measured[k] for k in ("mean_re", "mean_im", "rms", "clipped")]), want_measured), block_ms
            assert ing.level == level
            # the cursor is where it was: the next block is the one that would have come, conditioned
            f1, b1 = _next(eng, ing)
            assert (f0, f1) == (0, block_ms) and _same(b1, _numpy_condition(x[f1 * n:(f1 + block_ms) * n], level))
            # a second calibration measures the unconditioned output again
            again, _ = ing.calibrate(first_ms=5, n_ms=20, target_rms=target)
            nxt = ing.next_device_block()
            assert again == level and (nxt is None if 2 * block_ms >= 40 else nxt[0] == 2 * block_ms)
            # without an offset's removal the level is another one, and the last whole range is allowed
            flat, _ = ing.calibrate(first_ms=35, n_ms=5, target_rms=target, remove_dc=False)
            assert flat.dc_re == 0 and flat.dc_im == 0 and flat.gain < level.gain / 5
            for first_ms, n_ms in ((-1, 5), (36, 5), (40, 1), (0, 0), (0, 10001), (0, 41)):
                with pytest.raises(_lib.GypsumHipError, match="gyp_ingest_calibrate") as e:
                    ing.calibrate(first_ms=first_ms, n_ms=n_ms, target_rms=target)
                assert e.value.code == BAD
            with pytest.raises(_lib.GypsumHipError, match="target_rms"):
                ing.calibrate(first_ms=0, n_ms=5, target_rms=0.0)
            assert ing.level == flat                          # a refused call leaves the level alone
        finally:
            ing.close()


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene")
    w8, u8, q = model.offset_binary_scene(12)
    np.concatenate([w8, np.zeros(2, np.int8)]).tofile(d / "scene.i8")
    np.concatenate([u8, np.full(2, 128, np.uint8)]).tofile(d / "scene.u8")
    return d / "scene.u8", d / "scene.i8"


def _acquire_first_block(eng, ing, keep_samples=False):
    """gyp_acquire_dev over the handle's next block, straight from HBM: 32 records (and the block's samples)."""
    f, n_ms, dev = ing.next_device_block()
    assert (f, n_ms) == (0, 10)
    d_out = eng.alloc(32 * _lib.ACQ_RESULT.itemsize)
    eng.acquire_dev(dev, 1, n_ms * ing.n, n_ms, list(range(1, 33)), d_out.ptr.value)
    out = d_out.download(_lib.ACQ_RESULT, 32)
    d_out.free()
    x = None
    if keep_samples:
        x = np.empty(n_ms * ing.n, dtype=np.complex64)
        eng._check(eng.lib.gyp_memcpy_d2h(eng.ctx, _lib.ptr(x), _lib.C.c_void_p(dev), x.nbytes))
    return out, x


def _planted_found(records) -> bool:
    by_sat = {int(r["sat_id"]): r for r in records}
    absent = max(float(r["strength"]) for sv, r in by_sat.items() if sv not in model.SCENE_SATS)
    return all(int(by_sat[sv]["code_phase"]) == cp and float(by_sat[sv]["strength"]) > absent for sv, (cp, _) in model.SCENE_SATS.items())


def test_an_offset_binary_recording_is_acquired_once_its_level_is_set(engines, scene_files):
    eng = engines(model.SCENE_FS)
    rec, twin = scene_files
    kw = dict(block_ms=10, depth=3, engine=eng)
    a, b = IqFileIngest(rec, model.SCENE_FS, np.uint8, **kw), IqFileIngest(twin, model.SCENE_FS, np.int8, **kw)
    try:
        # (a) the int8 twin: the three planted satellites at their code phases, each stronger than every absent one
        b.set_scale(G)
        twin_records, _ = _acquire_first_block(eng, b)
        assert _planted_found(twin_records), twin_records
        for sv, (_, doppler) in model.SCENE_SATS.items():
            assert abs(int(twin_records[sv - 1]["doppler_hz"]) - doppler) <= 350      # half a bin of the coarsest level
        # (d) the uint8 words as they are: the float64 oracle says what the samples hold, the device must say the same
        raw_records, x = _acquire_first_block(eng, a, keep_samples=True)
        assert x.real.min() >= 1 and x.real.max() <= 255
        chips = orc.generate_ca_codes()
        weakest_twin = min(float(twin_records[sv - 1]["strength"]) for sv in model.SCENE_SATS)
        for sv, (cp, _) in model.SCENE_SATS.items():
            o = orc.acquire_satellite(sv, x.astype(np.complex128), model.SCENE_FS, model.SCENE_N, orc.prn_as_complex(chips[sv - 1], model.SCENE_N))
            r = raw_records[sv - 1]
            print(f"PRN {sv}: oracle code phase {o.prn_phase_shift} strength {o.correlation_strength:.2f}; device {int(r['code_phase'])} "
                  f"{float(r['strength']):.2f}; planted {cp}")
            assert (o.prn_phase_shift == cp) == (int(r["code_phase"]) == cp), sv
            assert (o.correlation_strength < weakest_twin) == (float(r["strength"]) < weakest_twin), sv
        # (b) the level {128, 128, g}: the twin's records, byte for byte
        a.set_level(IqLevel(128.0, 128.0, G))
        a.seek(0)
        assert _same(_acquire_first_block(eng, a)[0], twin_records)
        # (c) calibrated on its first 10 ms
        a.seek(0)
        level, measured = a.calibrate(0, 10, remove_dc=True)
        assert abs(level.dc_re - 128.0) < 0.5 and abs(level.dc_im - 128.0) < 0.5 and abs(measured["rms"] - 20.0) < 0.5
        assert abs(level.gain * measured["rms"] - default_target_rms(model.SCENE_N)) < 1e-7
        assert _planted_found(_acquire_first_block(eng, a)[0])
    finally:
        a.close()
        b.close()


def test_the_provider_serves_the_calibrated_handles_samples(engines, tmp_path):
    """An RTL-SDR style recording: uint8 at 2.048 Msps, resampled to 2.046 Msps, calibrated once after opening."""
    eng = engines(2_046_000)
    rng = np.random.default_rng(2048)
    path = tmp_path / "rtl.u8"
    np.clip(np.rint(rng.normal(127.4, 18.0, 2 * (12 * 2048 + 1))), 0, 255).astype(np.uint8).tofile(path)
    cal = dict(first_ms=0, n_ms=8, target_rms=0.05)
    prov = AntennaSampleProviderResampled(path, 2_048_000, sample_component_data_type=np.uint8, block_ms=5, engine=eng, calibrate=cal)
    ing = IqFileIngest(path, 2_046_000, np.uint8, block_ms=5, depth=3, engine=eng, resample_from_hz=2_048_000)
    try:
        level, _ = ing.calibrate(**cal)
        assert prov.level == level and abs(level.dc_re - 127.4) < 1.0
        _, want = _drain(eng, ing)
        got = prov.get_block(12).samples
        assert prov.total_ms == 12 and _same(got, want)
        assert abs(np.sqrt(np.mean(np.abs(got.astype(np.complex128)) ** 2)) - 0.05) < 0.002 and abs(got.mean()) < 0.002
        with pytest.raises(ValueError, match="exclude"):
            AntennaSampleProviderResampled(path, 2_048_000, sample_component_data_type=np.uint8, engine=eng, level=level, calibrate=cal)
        fixed = AntennaSampleProviderResampled(path, 2_048_000, sample_component_data_type=np.uint8, block_ms=5, engine=eng, level=level)
        assert _same(fixed.get_block(12).samples, want)
        fixed.close()
    finally:
        prov.close()
        ing.close()
