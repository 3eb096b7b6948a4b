"""Narrowband interference on the device (gyp_iq_tones_dev, gyp_notch_iq_dev, gyp_ingest_set_notches / _find_tones): the records and
the notched samples against the float64 model of tests/notch_model.py within derived bounds, bit-identical for every call shape,
window, alignment, grid size and residual store (LDS or the output buffer); the suppression against the model's own; the tones of
the gated scene found in int8 and uint8 files whatever the blocks; the chain order producer -> notches -> level; and a scene whose
satellites the detector misses under a CW 40 dB above the noise, acquired and tracked once the tone is found and removed."""
from __future__ import annotations

import numpy as np
import pytest

import notch_model as model
from gypsum_amd import _lib
from gypsum_amd.antenna_sample_provider import AntennaSampleProviderResampled
from gypsum_amd.engine import GypsumEngine
from gypsum_amd.ingest import IqFileIngest
from gypsum_amd.level import IqLevel, default_target_rms, level_from_stats
from gypsum_amd.notch import TONE_DTYPE, as_complex
from oracle import gypsum_oracle as orc

pytestmark = pytest.mark.gpu

BAD = _lib.GYP_E_BAD_ARG
RTOL_MAG = 1e-4          # tests/test_gpu_parity.py's bar for magnitudes and strengths
BIG = 2 ** 40 + 17


@pytest.fixture(scope="module")
def eng():
    e = GypsumEngine(0)
    e.set_stream_format(model.SCENE_FS, model.SCENE_N)
    yield e
    e.close()


def _same(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _tones(eng, flat, offset, n_streams, stride, first_index, n_blocks, block, fs, freqs, window):
    """gyp_iq_tones_dev on complex64 `flat` uploaded as it is, the first stream starting `offset` samples into the buffer."""
    assert offset + (n_streams - 1) * stride + n_blocks * block <= flat.size      # the kernel reads nothing else
    d_iq = eng.alloc(flat.nbytes).upload(flat)
    count = n_streams * n_blocks * len(freqs)
    d_out = eng.alloc(count * TONE_DTYPE.itemsize)
    eng.iq_tones_dev(d_iq.ptr.value + 8 * offset, n_streams, stride, first_index, n_blocks, block, fs, freqs, window, d_out.ptr.value)
    out = d_out.download(TONE_DTYPE, count).reshape(n_streams, n_blocks, len(freqs))
    d_iq.free()
    d_out.free()
    return out


def _notch(eng, flat, offset, n_streams, stride, first_index, n_ms, n, fs, tones, in_place):
    """(output buffer, input buffer) after gyp_notch_iq_dev, whole buffers downloaded; out of place the output starts as NaN."""
    assert offset + (n_streams - 1) * stride + n_ms * n <= flat.size
    d_in = eng.alloc(flat.nbytes).upload(flat)
    d_out = d_in if in_place else eng.alloc(flat.nbytes).upload(np.full(flat.size, np.nan + 0j, dtype=np.complex64))
    eng.notch_iq_dev(d_in.ptr.value + 8 * offset, d_out.ptr.value + 8 * offset, n_streams, stride, first_index, n_ms, n, fs, tones)
    out, src = d_out.download(np.complex64, flat.size), d_in.download(np.complex64, flat.size)
    d_in.free()
    if not in_place:
        d_out.free()
    return out, src


def _signal(rng, count, fs, first_index, tones, sigma):
    """Noise of `sigma` per component plus (Hz, amplitude) tones whose phase runs with the absolute index, complex64."""
    x = sigma * (rng.standard_normal(count) + 1j * rng.standard_normal(count))
    for k, (f, a) in enumerate(tones):
        x = x + a * model.mixer(f, first_index, count, fs) * np.exp(1j * (0.3 + k))
    return x.astype(np.complex64)


# the three streams of the shape tests: one without tones, one with two, one with eight (4 kHz apart at the closest)
LISTS = [[], [217_300, -403_000], [217_300, 221_300, -403_000, 0, 650_000, -15_000, 900_100, -820_000]]
AMPS = [[], [5.0, 0.5], [5.0, 2.0, 0.5, 1.0, 3.0, 0.7, 4.0, 1.5]]


def _three_streams(n, n_ms, first_index, seed):
    """(flat buffer, offset, stride, fs): stream s at offset + s * stride, a row start that is 8- but not 16-byte aligned (offset 1),
    a stride larger than n_ms * n and odd (so rows alternate between the two alignments)."""
    fs = n * 1000
    stride = n_ms * n + 3
    rng = np.random.default_rng(seed)
    flat = (rng.standard_normal(1 + 3 * stride) + 1j * rng.standard_normal(1 + 3 * stride)).astype(np.complex64)
    for s in range(3):
        a = 1 + s * stride
        flat[a:a + n_ms * n] = _signal(rng, n_ms * n, fs, first_index, list(zip(LISTS[s], AMPS[s])), 0.05 * (1 + 9 * s))
    return flat, 1, stride, fs


# ---------------------------------------------------------------------------------------------------- records
@pytest.mark.parametrize("first_index", [0, BIG])
@pytest.mark.parametrize("n", [2046, 4092])
def test_tone_records_equal_the_model_within_the_mixers_error(eng, n, first_index):
    """|A_dev - A_model| <= 2^-21 mean|x| per record: the only float32 quantity is the mixer, within 2^-22 of exact; the remaining
    factor of two covers the float64 reduction order.  Blocks of 1, 64, 1023 and N samples, both windows, 3 streams."""
    n_ms = 2
    flat, off, stride, fs = _three_streams(n, n_ms, first_index, n + first_index % 1000)
    freqs = [217_300, -403_000, 12_345]
    for block in (1, 64, 1023, n):
        n_blocks = n_ms * n // block
        for window in (model.RECT, model.HANN):
            got = as_complex(_tones(eng, flat, off, 3, stride, first_index, n_blocks, block, fs, freqs, window))
            worst = 0.0
            for s in range(3):
                x = flat[off + s * stride:off + s * stride + n_blocks * block]
                want = model.tones(x, fs, freqs, block, window, first_index)
                bound = 2.0 ** -21 * np.abs(x.astype(np.complex128)).reshape(n_blocks, block).mean(axis=1)
                err = np.abs(got[s] - want)
                worst = max(worst, float((err / bound[:, None]).max()))
                assert (err <= bound[:, None]).all(), (n, first_index, block, window, s, float((err / bound[:, None]).max()))
            print(f"N {n} first {first_index} block {block} window {window}: worst error / bound {worst:.3f}")
    # the strong tone is seen at its amplitude
    a = as_complex(_tones(eng, flat, off, 3, stride, first_index, n_ms, n, fs, [217_300], model.RECT))
    assert abs(abs(a[1, 0, 0]) - 5.0) < 0.05 and abs(a[0, 0, 0]) < 0.05


def test_tone_records_are_the_same_bits_for_every_call_shape(eng):
    """Two runs; a sub-window of the same buffer (blocks 5.. of stream 1 alone, its first index moved along); one stream at a time;
    the same samples 16-byte aligned; more items than the grid holds against a call that fits it."""
    n, n_ms, block = 2046, 2, 64
    flat, off, stride, fs = _three_streams(n, n_ms, BIG, 64)
    freqs = list(range(-400_000, 400_001, 50_000))
    n_blocks = n_ms * n // block
    for window in (model.RECT, model.HANN):
        got = _tones(eng, flat, off, 3, stride, BIG, n_blocks, block, fs, freqs, window)
        assert _same(_tones(eng, flat, off, 3, stride, BIG, n_blocks, block, fs, freqs, window), got)
        sub = _tones(eng, flat, off + stride + 5 * block, 1, 0, BIG + 5 * block, 7, block, fs, freqs, window)
        assert _same(sub[0], got[1, 5:12]), window
        for s in range(3):
            assert _same(_tones(eng, flat, off + s * stride, 1, 0, BIG, n_blocks, block, fs, freqs, window)[0], got[s]), (window, s)
        moved = np.ascontiguousarray(flat[off + stride:off + stride + n_blocks * block])          # row start 16-byte aligned
        assert _same(_tones(eng, moved, 0, 1, 0, BIG, n_blocks, block, fs, freqs, window)[0], got[1]), window
        assert _same(_tones(eng, flat, off, 3, stride, BIG, n_blocks, block, fs, freqs[3:4], window)[:, :, 0], got[:, :, 3]), window


def test_tones_arguments_are_checked(eng):
    d = eng.alloc(1 << 16)
    p, fs = d.ptr.value, 2_046_000
    ok = dict(iq=p, ns=1, stride=64, first=0, nb=1, block=64, fs=fs, freqs=[1000], window=0, out=p)
    cases = {"iq NULL": dict(iq=0), "out NULL": dict(out=0), "n_streams 0": dict(ns=0), "n_blocks 0": dict(nb=0), "block 0": dict(block=0),
             "first < 0": dict(first=-1), "stride": dict(ns=2, stride=63), "fs 0": dict(fs=0), "fs 2^31": dict(fs=2 ** 31),
             "f = fs/2": dict(freqs=[fs // 2]), "f = -fs/2": dict(freqs=[-(fs // 2)]), "window 2": dict(window=2)}
    for what, change in cases.items():
        a = dict(ok, **change)
        with pytest.raises(_lib.GypsumHipError, match="gyp_iq_tones_dev") as e:
            eng.iq_tones_dev(a["iq"], a["ns"], a["stride"], a["first"], a["nb"], a["block"], a["fs"], a["freqs"], a["window"], a["out"])
        assert e.value.code == BAD, what
    eng.iq_tones_dev(p, 1, 64, 0, 1, 64, fs, [fs // 2 - 1, -(fs // 2 - 1)], 1, p + 4096)
    eng.sync()
    d.free()


# ---------------------------------------------------------------------------------------------------- notched samples
def _assert_notched_within_bound(got, x, fs, n, tones, first_index, what):
    """Per component |y_dev - y_model| <= sum_t 2^-20 |A_t| + 2^-23 |x|: the mixer's error enters once in the measurement and once in
    the subtraction of every tone, and then there is a float32 rounding."""
    want, amps = model.notch(x, fs, n, tones, first_index)
    bound = np.repeat(2.0 ** -20 * np.abs(amps).sum(axis=1), n) + 2.0 ** -23 * np.abs(x.astype(np.complex128))
    g = got.astype(np.complex128)
    err = np.maximum(np.abs(g.real - want.real), np.abs(g.imag - want.imag))
    print(f"{what}: worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), (what, float((err / bound).max()))
    return want


@pytest.mark.parametrize("first_index", [0, BIG])
@pytest.mark.parametrize("n", [2046, 4092])
def test_notched_samples_equal_the_model_in_place_and_out_of_place(eng, n, first_index):
    n_ms = 3
    flat, off, stride, fs = _three_streams(n, n_ms, first_index, 3 * n + first_index % 1000)
    outs = {}
    for in_place in (False, True):
        out, src = _notch(eng, flat, off, 3, stride, first_index, n_ms, n, fs, LISTS, in_place)
        touched = np.zeros(flat.size, dtype=bool)
        for s in range(3):
            a = off + s * stride
            touched[a:a + n_ms * n] = True
            _assert_notched_within_bound(out[a:a + n_ms * n], flat[a:a + n_ms * n], fs, n, LISTS[s], first_index, f"N {n} stream {s} in place {in_place}")
        assert _same(out[off:off + n_ms * n], flat[off:off + n_ms * n])            # the empty list returns the input bits
        if in_place:
            assert _same(out[~touched], flat[~touched])
        else:
            assert np.isnan(out[~touched].real).all() and _same(src, flat)
        outs[in_place] = out[touched]
    assert _same(outs[False], outs[True])
    # the strong tone of stream 2 is gone: what is left at its frequency is the noise's share
    y = outs[True][2 * n_ms * n:]
    left = abs(model.tones(y, fs, [217_300], n_ms * n, model.RECT, first_index)[0, 0])
    assert left < 5.0 * 10 ** (-40 / 20), left


def test_notched_samples_are_the_same_bits_for_every_call_shape_and_residual_store(eng):
    """A sub-window (millisecond 1 of stream 2 alone), one stream at a time, one millisecond at a time, 16-byte aligned rows, 1 and 8
    workgroups per CU, and the residual kept in the output buffer instead of LDS (gyp_debug_set notch_no_lds)."""
    n, n_ms = 2046, 3
    flat, off, stride, fs = _three_streams(n, n_ms, BIG, 2046)
    got, _ = _notch(eng, flat, off, 3, stride, BIG, n_ms, n, fs, LISTS, False)

    def rows(out, a, count):
        return out[a:a + count]

    for s in range(3):
        a = off + s * stride
        one, _ = _notch(eng, flat, a, 1, 0, BIG, n_ms, n, fs, [LISTS[s]], True)
        assert _same(rows(one, a, n_ms * n), rows(got, a, n_ms * n)), s
        for m in range(n_ms):
            ms, _ = _notch(eng, flat, a + m * n, 1, 0, BIG + m * n, 1, n, fs, [LISTS[s]], False)
            assert _same(rows(ms, a + m * n, n), rows(got, a + m * n, n)), (s, m)
    a = off + 2 * stride
    moved = np.ascontiguousarray(flat[a:a + n_ms * n])
    assert _same(_notch(eng, moved, 0, 1, 0, BIG, n_ms, n, fs, [LISTS[2]], True)[0], rows(got, a, n_ms * n))
    try:
        for per_cu in (1, 8):
            eng.debug_set("widen_wg_per_cu", per_cu)
            assert _same(_notch(eng, flat, off, 3, stride, BIG, n_ms, n, fs, LISTS, False)[0], got), per_cu
    finally:
        eng.debug_set("widen_wg_per_cu", 2)
    try:
        eng.debug_set("notch_no_lds", 1)
        for in_place in (False, True):
            other, _ = _notch(eng, flat, off, 3, stride, BIG, n_ms, n, fs, LISTS, in_place)
            for s in range(3):
                a = off + s * stride
                assert _same(rows(other, a, n_ms * n), rows(got, a, n_ms * n)), (in_place, s)
    finally:
        eng.debug_set("notch_no_lds", 0)
    assert eng.debug_get("notch_no_lds") == 0


def test_the_rate_that_does_not_fit_lds_is_notched_from_the_output_buffer(eng):
    """N = 49104 (393 KiB per millisecond), 2 ms, 2 streams: against the model, and a sub-window bit for bit."""
    n, n_ms, fs = 49104, 2, 49_104_000
    stride = n_ms * n + 1
    rng = np.random.default_rng(49104)
    lists = [[2_173_000, -9_000_000, 21_000_000], [0]]
    flat = np.zeros(1 + 2 * stride, dtype=np.complex64)
    flat[1:1 + n_ms * n] = _signal(rng, n_ms * n, fs, BIG, [(2_173_000, 5.0), (-9_000_000, 1.0), (21_000_000, 0.3)], 0.05)
    flat[1 + stride:1 + stride + n_ms * n] = _signal(rng, n_ms * n, fs, BIG, [(0, 2.0)], 0.5)
    outs = []
    for in_place in (False, True):
        out, _ = _notch(eng, flat, 1, 2, stride, BIG, n_ms, n, fs, lists, in_place)
        for s in range(2):
            a = 1 + s * stride
            _assert_notched_within_bound(out[a:a + n_ms * n], flat[a:a + n_ms * n], fs, n, lists[s], BIG, f"N {n} stream {s} in place {in_place}")
        outs.append(out)
    assert _same(outs[0][1:1 + n_ms * n], outs[1][1:1 + n_ms * n])
    sub, _ = _notch(eng, flat, 1 + n, 1, 0, BIG + n, 1, n, fs, [lists[0]], False)
    assert _same(sub[1 + n:1 + 2 * n], outs[0][1 + n:1 + 2 * n])


def test_bad_tone_lists_are_refused(eng):
    d = eng.alloc(1 << 16)
    p, fs, n = d.ptr.value, 2_046_000, 2046

    def refused(tones, what, **kw):
        a = dict(inp=p, out=p, ns=1, stride=n, first=0, n_ms=1, n=n, fs=fs)
        a.update(kw)
        with pytest.raises(_lib.GypsumHipError, match="gyp_notch_iq_dev") as e:
            eng.notch_iq_dev(a["inp"], a["out"], a["ns"], a["stride"], a["first"], a["n_ms"], a["n"], a["fs"], tones)
        assert e.value.code == BAD, what

    nine = np.zeros(1, dtype=_lib.NOTCH_TONES)
    nine["count"] = 9
    refused(nine, "K = 9")
    refused([[100_000, 103_999]], "3999 Hz apart")
    refused([[100_000, 200_000, 96_001]], "3999 Hz apart, out of order")
    refused([[100_000, 100_000]], "the same tone twice")
    refused([[fs // 2]], "f = fs / 2")
    refused([[-(fs // 2)]], "f = -fs / 2")
    reserved = np.zeros(1, dtype=_lib.NOTCH_TONES)
    reserved["reserved"] = 1
    refused(reserved, "reserved")
    refused([[1000]], "in NULL", inp=0)
    refused([[1000]], "out NULL", out=0)
    refused([[1000]], "first < 0", first=-1)
    refused([[1000]], "N 0", n=0)
    refused([[1000]], "fs 0", fs=0)
    refused([[1000], [1000]], "stride", ns=2, stride=n - 1)
    assert eng.lib.gyp_notch_iq_dev(eng.ctx, p, p, 1, n, 0, 1, n, fs, None) == BAD
    eng.notch_iq_dev(p, p, 1, n, 0, 1, n, fs, [[100_000, 104_000]])              # 4000 Hz apart is allowed
    eng.notch_iq_dev(p, p, 1, n, 0, 0, n, fs, [[100_000]])                       # nothing to do
    eng.sync()
    d.free()


# ---------------------------------------------------------------------------------------------------- suppression
@pytest.mark.parametrize("offset_hz", [0.0, 0.4])
def test_suppression_is_the_models(eng, offset_hz):
    """Residual power in +-500 Hz around the tone, measured in float64 on the device's output, lies within 1 dB of what the model's
    own output leaves on the same input: a tone on its listed frequency and one 0.4 Hz off it."""
    x, _ = model.scene(10, tone_offset_hz=offset_hz)
    fs, n, f = model.SCENE_FS, model.SCENE_N, model.SCENE_TONE_HZ
    got = eng.notch_iq(x, fs, n, [f])
    want, _ = model.notch(x, fs, n, [f])
    before, dev, ref = (model.band_power(v, fs, f) for v in (x, got, want))
    print(f"tone {offset_hz} Hz off its listed frequency: suppression in +-500 Hz {10 * np.log10(before / dev):.2f} dB on the device, "
          f"{10 * np.log10(before / ref):.2f} dB in the float64 model")
    assert abs(10 * np.log10(dev / ref)) <= 1.0
    assert 10 * np.log10(before / dev) > 30.0


# ---------------------------------------------------------------------------------------------------- ingest
def _drain(eng, ing):
    got, firsts = [], []
    while (blk := ing.next_device_block()) is not None:
        f, count, dev = blk
        buf = np.empty(count * ing.n, dtype=np.complex64)
        eng._check(eng.lib.gyp_memcpy_d2h(eng.ctx, _lib.ptr(buf), _lib.C.c_void_p(dev), buf.nbytes))
        got.append(buf)
        firsts.append(f)
    return firsts, (np.concatenate(got) if got else np.empty(0, np.complex64))


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    """The gated scene over 12 ms as int8 and uint8 (offset 128) words, its clean twin, and a scene with three tones."""
    d = tmp_path_factory.mktemp("notch")
    x, clean = model.scene(12)
    three, _ = model.scene(12, tone_hz=(217_300, -640_000, 455_500), tone_db=(30.0, 40.0, 20.0))
    w8, u8, q = model.scene_words(x)
    files = {"x": x, "q": q}
    for name, data in (("tone", x), ("clean", clean), ("three", three)):
        a8, b8, _ = model.scene_words(data, q=q if name != "three" else None)
        np.concatenate([a8, np.zeros(2, np.int8)]).tofile(d / f"{name}.i8")
        np.concatenate([b8, np.full(2, 128, np.uint8)]).tofile(d / f"{name}.u8")
        files[name] = {np.int8: d / f"{name}.i8", np.uint8: d / f"{name}.u8"}
    return files


@pytest.mark.parametrize("dtype", [np.int8, np.uint8])
def test_find_tones_finds_the_scenes_tone_whatever_the_blocks(eng, scene_files, dtype):
    """Exactly one tone within 2 Hz of 217 300 in the int8 and in the offset-binary file (whose offset at 0 Hz is not reported),
    the same for block_ms 1, 7 and 100; none in the clean twin; three planted tones strongest first."""
    fs = model.SCENE_FS
    results = []
    for block_ms in (1, 7, 100):
        ing = IqFileIngest(scene_files["tone"][dtype], fs, dtype, block_ms=block_ms, depth=3, engine=eng)
        try:
            assert ing.total_ms == 12 and ing.notches == []
            first = ing.next_device_block()[0]
            tones = ing.find_tones(first_ms=1, n_ms=10, install=False)
            assert ing.notches == []
            assert len(tones) == 1 and abs(tones[0][0] - model.SCENE_TONE_HZ) <= 2, (block_ms, tones)
            assert tones[0][1] > 40.0                                  # dB over the spectrum's median
            nxt = ing.next_device_block()                               # the cursor is where it was
            assert first == 0 and (nxt is None if block_ms >= 12 else nxt[0] == block_ms)
            installed = ing.find_tones(first_ms=1, n_ms=10)
            assert installed == tones and ing.notches == [tones[0][0]]
            results.append(tones)
            for first_ms, n_ms in ((-1, 5), (8, 5), (0, 0), (0, 1001)):
                with pytest.raises(_lib.GypsumHipError, match="gyp_ingest_find_tones") as e:
                    ing.find_tones(first_ms=first_ms, n_ms=n_ms)
                assert e.value.code == BAD
            with pytest.raises(_lib.GypsumHipError, match="gyp_ingest_find_tones"):
                ing.find_tones(threshold=0.0)
            assert ing.notches == [tones[0][0]]                         # a refused call leaves the notches alone
        finally:
            ing.close()
    assert results[0] == results[1] == results[2]
    ing = IqFileIngest(scene_files["clean"][dtype], fs, dtype, block_ms=7, depth=3, engine=eng)
    try:
        assert ing.find_tones(first_ms=0, n_ms=10) == [] and ing.notches == []
    finally:
        ing.close()
    ing = IqFileIngest(scene_files["three"][dtype], fs, dtype, block_ms=7, depth=3, engine=eng)
    try:
        tones = ing.find_tones(first_ms=0, n_ms=10)
        assert [abs(f - want) <= 2 for (f, _), want in zip(tones, (-640_000, 217_300, 455_500))] == [True] * 3 and len(tones) == 3, tones
        assert tones[0][1] > tones[1][1] > tones[2][1]
        assert ing.find_tones(first_ms=0, n_ms=10, max_tones=2, install=False) == tones[:2]
    finally:
        ing.close()


@pytest.mark.parametrize("block_ms", [1, 7])
def test_a_handles_blocks_are_notched_as_one_call_would(eng, scene_files, block_ms):
    """Block by block through an ingest handle, after a seek and set between two blocks: the bits of one gyp_notch_iq_dev call over
    the handle's plain output; an empty list is the handle without the feature; host blocks are refused while notches are on."""
    fs, n = model.SCENE_FS, model.SCENE_N
    tones = [model.SCENE_TONE_HZ, -300_000]
    ing = IqFileIngest(scene_files["tone"][np.int8], fs, np.int8, block_ms=block_ms, depth=3, engine=eng)
    try:
        ing.set_scale(0.01)
        firsts, plain = _drain(eng, ing)
        assert plain.size == 12 * n
        want = eng.notch_iq(plain, fs, n, tones)
        assert not _same(want, plain)
        ing.set_notches(tones)
        assert ing.notches == tones
        for at in (0, 5):
            ing.seek(at)
            firsts2, got = _drain(eng, ing)
            assert firsts2 == [f for f in range(at, 12, block_ms)] and _same(got, want[at * n:]), (block_ms, at)
        with pytest.raises(_lib.GypsumHipError, match="gyp_ingest_next_host") as e:
            ing.next_host_block()
        assert e.value.code == BAD
        with pytest.raises(_lib.GypsumHipError, match="gyp_ingest_set_notches"):
            ing.set_notches([100_000, 103_999])
        assert ing.notches == tones
        # set between two blocks: the block uploaded ahead is dropped and read again
        ing.set_notches([])
        ing.seek(0)
        f0, c0, dev = ing.next_device_block()
        b0 = np.empty(c0 * n, dtype=np.complex64)
        eng._check(eng.lib.gyp_memcpy_d2h(eng.ctx, _lib.ptr(b0), _lib.C.c_void_p(dev), b0.nbytes))
        ing.set_notches(tones)
        f1, c1, dev = ing.next_device_block()
        b1 = np.empty(c1 * n, dtype=np.complex64)
        eng._check(eng.lib.gyp_memcpy_d2h(eng.ctx, _lib.ptr(b1), _lib.C.c_void_p(dev), b1.nbytes))
        assert (f0, f1) == (0, block_ms) and _same(b0, plain[:c0 * n]) and _same(b1, want[f1 * n:(f1 + c1) * n])
        ing.set_notches(None)
        ing.seek(0)
        assert _same(_drain(eng, ing)[1], plain) and ing.notches == []
        ing.seek(0)
        assert ing.next_host_block() is not None
    finally:
        ing.close()


def test_the_level_is_measured_behind_the_notches(eng, scene_files):
    """Chain order producer -> notches -> level: with notches installed, calibrate installs level_from_stats of the NOTCHED output's
    statistics, and the blocks are condition(notch(plain)); without notches it is the level of the plain output."""
    fs, n = model.SCENE_FS, model.SCENE_N
    ing = IqFileIngest(scene_files["tone"][np.uint8], fs, np.uint8, block_ms=7, depth=3, engine=eng)
    try:
        _, plain = _drain(eng, ing)
        ing.seek(0)
        jammed, _ = ing.calibrate(first_ms=0, n_ms=10)
        ing.set_level(None)
        tones = [f for f, _ in ing.find_tones(first_ms=0, n_ms=10)]
        notched = eng.notch_iq(plain, fs, n, tones)
        want, _ = level_from_stats(eng.iq_stats(notched[:10 * n], n), n, default_target_rms(n))
        level, measured = ing.calibrate(first_ms=0, n_ms=10)
        assert level == want and ing.level == level and ing.notches == tones
        assert level.gain > 20 * jammed.gain                           # the jammed level was 40 dB off
        assert abs(level.dc_re - 128.0) < 0.5 and abs(level.dc_im - 128.0) < 0.5
        ing.seek(0)
        assert _same(_drain(eng, ing)[1], eng.condition_iq(notched, level))
    finally:
        ing.close()


def test_a_failed_measurement_restores_the_level_the_notches_and_the_cursor(eng, tmp_path):
    """An error past the point where calibrate / find_tones have switched the conditioning off: a float32 recording (uploaded as it
    is) with one NaN word in millisecond 6 makes the statistics and the scan's spectrum not finite.  After each failed call the level
    and the notches are the installed ones, and the blocks handed out afterwards are those of a twin handle nothing was asked of."""
    fs, n, n_ms = model.SCENE_FS, model.SCENE_N, 12
    words = np.random.default_rng(6).standard_normal((n_ms * n + 1) * 2).astype(np.float32)
    words[2 * (6 * n + 100)] = np.nan
    path = tmp_path / "nan.f32"
    words.tofile(path)
    level, tones = IqLevel(0.25, -0.5, 2.0), [100_000, -300_000]
    subject, twin = (IqFileIngest(path, fs, np.float32, block_ms=2, depth=3, engine=eng) for _ in range(2))

    def block(ing):
        f, count, dev = ing.next_device_block()
        buf = np.empty(count * n, dtype=np.complex64)
        eng._check(eng.lib.gyp_memcpy_d2h(eng.ctx, _lib.ptr(buf), _lib.C.c_void_p(dev), buf.nbytes))
        return f, count, buf.view(np.uint32)

    try:
        for ing in (subject, twin):
            assert ing.total_ms == n_ms
            ing.set_level(level)
            ing.set_notches(tones)
        first = [block(ing) for ing in (subject, twin)]
        assert first[0][:2] == first[1][:2] == (0, 2) and _same(first[0][2], first[1][2])
        for call, text in ((subject.calibrate, "gyp_ingest_calibrate"), (subject.find_tones, "the scan's spectrum")):
            with pytest.raises(_lib.GypsumHipError, match=text) as e:
                call(first_ms=4, n_ms=4)
            assert e.value.code == BAD
            assert subject.level == level and subject.notches == tones
        found = subject.find_tones(first_ms=0, n_ms=4, install=False)                 # no NaN there: returns normally
        assert isinstance(found, list) and subject.level == level and subject.notches == tones
        for want_first in range(2, n_ms, 2):
            a, b = block(subject), block(twin)
            assert a[:2] == b[:2] == (want_first, 2) and _same(a[2], b[2]), want_first
        assert subject.next_device_block() is None and twin.next_device_block() is None
        assert np.isnan(words[2 * 6 * n:2 * 7 * n]).sum() == 1
    finally:
        subject.close()
        twin.close()


def test_the_provider_finds_and_installs_the_tones_before_it_calibrates(eng, tmp_path):
    """An RTL-SDR style recording: uint8 at 2.048 Msps with a spur, resampled to 2.046 Msps."""
    rng = np.random.default_rng(2048)
    count = 12 * 2048 + 1
    x = 1.5 * (rng.standard_normal(count) + 1j * rng.standard_normal(count)) + 100.0 * np.exp(2j * np.pi * 333_333.0 / 2_048_000 * np.arange(count))
    words = np.empty(2 * count)
    words[0::2], words[1::2] = x.real + 127.4, x.imag + 127.4
    path = tmp_path / "rtl.u8"
    np.clip(np.rint(words), 0, 255).astype(np.uint8).tofile(path)
    kw = dict(sample_component_data_type=np.uint8, block_ms=5, engine=eng)
    prov = AntennaSampleProviderResampled(path, 2_048_000, find_tones=True, calibrate=dict(first_ms=0, n_ms=8), **kw)
    ing = IqFileIngest(path, 2_046_000, np.uint8, block_ms=5, depth=3, engine=eng, resample_from_hz=2_048_000)
    try:
        assert len(prov.tones) == 1 and abs(prov.tones[0][0] - 333_333) <= 2 and prov.notches == [prov.tones[0][0]]
        assert ing.find_tones() == prov.tones
        level, _ = ing.calibrate(first_ms=0, n_ms=8)
        assert prov.level == level
        got = prov.get_block(12).samples
        assert _same(got, _drain(eng, ing)[1])
        assert abs(np.sqrt(np.mean(np.abs(got.astype(np.complex128)) ** 2)) - default_target_rms(2046)) < 0.05 * default_target_rms(2046)
        fixed = AntennaSampleProviderResampled(path, 2_048_000, notches=prov.notches, level=level, **kw)
        assert _same(fixed.get_block(12).samples, got)
        fixed.close()
        with pytest.raises(ValueError, match="exclude"):
            AntennaSampleProviderResampled(path, 2_048_000, notches=[1000], find_tones=True, **kw)
    finally:
        prov.close()
        ing.close()


# ---------------------------------------------------------------------------------------------------- end to end
def _acquire(eng, dev_ptr, n_ms, n, sats):
    d_out = eng.alloc(len(sats) * _lib.ACQ_RESULT.itemsize)
    eng.acquire_dev(dev_ptr, 1, n_ms * n, n_ms, sats, d_out.ptr.value)
    out = d_out.download(_lib.ACQ_RESULT, len(sats))
    d_out.free()
    return out


def test_a_jammed_recording_is_acquired_and_tracked_once_its_tone_is_found(eng, tmp_path):
    """The gated scene as a float32 recording.  Un-notched the detector misses planted satellites, as the gate says
    (tests/test_notch_host.py); with the tone found and installed the device's acquisition of the notched stream equals the oracle's
    acquisition of the model-notched stream (Doppler and code phase exact, strength within test_gpu_parity's tolerance), and 300 ms
    of tracking of the four channels give the oracle's pseudosymbols."""
    fs, n, n_track = model.SCENE_FS, model.SCENE_N, 300
    x, _ = model.scene(n_track)
    path = tmp_path / "jammed.f32"
    np.concatenate([x, np.zeros(1, np.complex64)]).view(np.float32).tofile(path)
    sats = list(model.SCENE_SATS)
    ing = IqFileIngest(path, fs, np.float32, block_ms=10, depth=3, engine=eng)
    try:
        f, n_ms, dev = ing.next_device_block()
        assert (f, n_ms) == (0, 10)
        raw = _acquire(eng, dev, 10, n, sats)
        missed = [sv for r, sv in zip(raw, sats) if int(r["code_phase"]) != model.SCENE_SATS[sv][0] or float(r["strength"]) <= 3.0]
        print("un-notched: missed", missed, [(int(r["doppler_hz"]), int(r["code_phase"]), round(float(r["strength"]), 2)) for r in raw])
        assert missed
        tones = ing.find_tones(first_ms=0, n_ms=10)
        assert len(tones) == 1 and abs(tones[0][0] - model.SCENE_TONE_HZ) <= 2
        ing.seek(0)
        f, n_ms, dev = ing.next_device_block()
        got = _acquire(eng, dev, 10, n, sats)
        ing.seek(0)
        ing2 = IqFileIngest(path, fs, np.float32, block_ms=n_track, depth=3, engine=eng)
        ing2.set_notches(ing.notches)
        _, notched = _drain(eng, ing2)
        ing2.close()
        assert notched.size == n_track * n
    finally:
        ing.close()
    want_stream, _ = model.notch(x, fs, n, [tones[0][0]])
    chips = orc.generate_ca_codes()
    inits = np.zeros(len(sats), dtype=_lib.CHAN_INIT)
    for i, sv in enumerate(sats):
        o = orc.acquire_satellite(sv, want_stream[:10 * n], fs, n, orc.prn_as_complex(chips[sv - 1], n))
        r = got[i]
        print(f"PRN {sv}: oracle {o.doppler_shift} {o.prn_phase_shift} {o.correlation_strength:.4f}; device {int(r['doppler_hz'])} "
              f"{int(r['code_phase'])} {float(r['strength']):.4f}")
        assert int(r["doppler_hz"]) == o.doppler_shift and int(r["code_phase"]) == o.prn_phase_shift == model.SCENE_SATS[sv][0]
        assert float(r["strength"]) == pytest.approx(o.correlation_strength, rel=RTOL_MAG) and o.correlation_strength > 3.0
        inits[i] = (0, sv, float(r["doppler_hz"]), float(r["carrier_phase"]), int(r["code_phase"]), 0)
    times = [orc.chunk_times(ms * n, n, fs) for ms in range(n_track)]
    bank = eng.create_bank(inits)
    rec = bank.track_block(notched, 1, n_track, [a for a, _ in times])
    bank.close()
    for i, sv in enumerate(sats):
        trk = orc.Tracker(orc.TrackingState(float(inits[i]["doppler_hz"]), float(inits[i]["carrier_phase"]), int(inits[i]["code_phase"])),
                          orc.prn_as_complex(chips[sv - 1], n), fs, n)
        rows = [trk.process_samples(want_stream[j * n:(j + 1) * n], st, en) for j, (st, en) in enumerate(times)]
        assert [int(v) for v in rec[i]["pseudosymbol"]] == [r.pseudosymbol for r in rows], sv
        assert [int(v) for v in rec[i]["status"]] == [0] * n_track
