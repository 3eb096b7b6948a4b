"""Pulsed interference on the device (gyp_blank_iq_dev, gyp_iq_power_hist_dev, gyp_ingest_set_blanker / _find_pulses / _last_blanked):
blanked samples, counts and histograms equal to the integers and bits of tests/blank_model.py for every size, alignment, guard, call
shape and grid size; the ingest handle's chain producer -> blanker -> notches -> level; and a scene whose satellites the detector
misses under pulses 30 dB above the noise, acquired and tracked once the pulses are found and blanked."""
from __future__ import annotations

import numpy as np
import pytest

import blank_model as model
import notch_model
from gypsum_amd import _lib
from gypsum_amd.antenna_sample_provider import AntennaSampleProviderResampled
from gypsum_amd.blanker import Blanker
from gypsum_amd.engine import GypsumEngine
from gypsum_amd.ingest import IqFileIngest
from gypsum_amd.level import IqLevel, default_target_rms, level_from_stats
from gypsum_amd.quality import SUMS_DTYPE, from_sums
from oracle import gypsum_oracle as orc

pytestmark = pytest.mark.gpu

BAD = _lib.GYP_E_BAD_ARG
RTOL_MAG = 1e-4          # tests/test_gpu_parity.py's bar for magnitudes and strengths
GUARDS = (0, 1, 4, 63, 64)


@pytest.fixture(scope="module")
def eng():
    e = GypsumEngine(0)
    e.set_stream_format(model.SCENE_FS, model.SCENE_N)
    yield e
    e.close()


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.complex64).view(np.uint64)


def _same(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _m(b: Blanker) -> model.Blanker:
    return model.Blanker(b.center_re, b.center_im, b.threshold, b.guard)


POISON = np.complex64(complex(np.nan, np.nan))


def _blank(eng, flat, offset, n_streams, stride, n_ms, n, blankers, in_place):
    """(output buffer, input buffer, counts[n_streams, n_ms]) after gyp_blank_iq_dev, whole buffers downloaded; out of place the
    output starts as NaN; the counts start as -1."""
    assert offset + (n_streams - 1) * stride + n_ms * n <= flat.size      # the kernel touches nothing else
    d_in = eng.alloc(flat.nbytes).upload(flat)
    d_out = d_in if in_place else eng.alloc(flat.nbytes).upload(np.full(flat.size, POISON, dtype=np.complex64))
    d_cnt = eng.alloc(4 * n_streams * n_ms + 4).upload(np.full(n_streams * n_ms + 1, -1, dtype=np.int32))
    eng.blank_iq_dev(d_in.ptr.value + 8 * offset, d_out.ptr.value + 8 * offset, n_streams, stride, n_ms, n, blankers, d_cnt.ptr.value)
    out, src = d_out.download(np.complex64, flat.size), d_in.download(np.complex64, flat.size)
    cnt = d_cnt.download(np.int32, n_streams * n_ms + 1)
    assert cnt[-1] == -1
    d_in.free()
    d_cnt.free()
    if not in_place:
        d_out.free()
    return out, src, cnt[:-1].reshape(n_streams, n_ms)


def _pulsed(count, seed, db=20.0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(count) + 1j * rng.standard_normal(count) + model.pulses(count, 1.0, seed + 1, period=409, width=41, db=db)
    return x.astype(np.complex64)


# ---------------------------------------------------------------------------------------------------- samples and counts
@pytest.mark.parametrize("offset", [0, 1], ids=["rows on 16 bytes", "rows 8 bytes off"])
@pytest.mark.parametrize("n,n_ms", [(1023, 3), (2046, 3), (4092, 3), (49104, 1)])
def test_blanked_samples_and_counts_equal_the_models_bits(eng, n, n_ms, offset):
    """N = 1023 is odd (rows alternate between the two alignments and end in half a pair); N = 2046 has 62 valid bits in its last
    hit word; N = 49104 has more chunks than a wavefront keeps in registers, so its tail is read a second time.  Two streams with their own blankers, guards 0, 1, 4, 63 and 64, in place and out of place; the buffer
    around the rows keeps its bits."""
    stride = n_ms * n + (2 if offset == 0 else 3)            # rows on 16 bytes stay there; the others alternate
    flat = _pulsed(offset + 2 * stride + 5, n)
    flat[offset + 7] = np.nan                                # a NaN sample in stream 0
    for guard in GUARDS:
        blankers = [Blanker(0.0, 0.0, 4.0, guard), Blanker(0.25, -0.5, 3.5, guard)]
        want = flat.copy()
        want_counts = np.zeros((2, n_ms), dtype=np.int32)
        touched = np.zeros(flat.size, dtype=bool)
        for s in range(2):
            a = offset + s * stride
            want[a:a + n_ms * n], want_counts[s] = model.blank(flat[a:a + n_ms * n], n, _m(blankers[s]))
            touched[a:a + n_ms * n] = True
        assert want_counts.min() > 0
        for in_place in (False, True):
            out, src, counts = _blank(eng, flat, offset, 2, stride, n_ms, n, blankers, in_place)
            what = (n, offset, guard, in_place)
            assert np.array_equal(counts, want_counts), (what, counts, want_counts)
            assert np.array_equal(_bits(out)[touched], _bits(want)[touched]), what
            if in_place:
                assert np.array_equal(_bits(out)[~touched], _bits(flat)[~touched]), what
            else:
                assert np.isnan(out[~touched].real).all() and np.array_equal(_bits(src), _bits(flat)), what


def test_constructed_milliseconds(eng):
    """One construction per millisecond of N = 2046 samples at 0.5 + 0.5j (p = 0.5) under a threshold of 3 (t2 = 9), guards 1 and
    64, rows on 16 bytes and 8 bytes off, in place and out of place: the model's bits, and what must hold spelled out."""
    n = 2046
    cases = {"a hit at sample 0": [0], "a hit at the last sample": [n - 1], "a hit at 63": [63], "a hit at 64": [64], "a hit at 127": [127],
             "a hit at 128": [128], "hits at 63 and 64": [63, 64], "p equals t2": [], "p one ulp below t2": [], "a NaN beside a hit": [1000],
             "every sample a hit": list(range(n)), "no hit": [], "a hit in the last sample, none in the next millisecond": [n - 1], "the next millisecond": []}
    names = list(cases)
    x = np.full(len(names) * n, 0.5 + 0.5j, dtype=np.complex64)
    for m, name in enumerate(names):
        x[m * n + np.asarray(cases[name], dtype=np.int64)] = 10.0
    below = np.nextafter(np.float32(3.0), np.float32(0.0))
    x[names.index("p equals t2") * n + 500] = 3.0
    x[names.index("p one ulp below t2") * n + 500] = below
    assert model.power(np.array([3.0], np.complex64))[0] == np.float32(9.0)
    assert model.power(np.array([below], np.complex64))[0] == np.nextafter(np.float32(9.0), np.float32(0.0))
    x[names.index("a NaN beside a hit") * n + 1003] = complex(np.nan, 1.0)
    for guard in (1, 64):
        b = Blanker(0.0, 0.0, 3.0, guard)
        want, want_counts = model.blank(x, n, _m(b))
        row = {name: want[m * n:(m + 1) * n] for m, name in enumerate(names)}
        cnt = dict(zip(names, want_counts.tolist()))
        # the model says what the header says
        assert cnt["a hit at sample 0"] == cnt["a hit at the last sample"] == guard + 1
        assert cnt["a hit at 63"] == min(63, guard) + 1 + guard and cnt["a hit at 64"] == cnt["a hit at 127"] == cnt["a hit at 128"] == 2 * guard + 1
        assert cnt["hits at 63 and 64"] == (64 + guard) - max(0, 63 - guard) + 1
        assert cnt["p equals t2"] == min(500, guard) + 1 + guard and cnt["p one ulp below t2"] == 0 and cnt["no hit"] == 0
        assert cnt["every sample a hit"] == n
        assert np.isnan(row["a NaN beside a hit"][1003].real) == (guard < 3)          # no hit itself; a guard of 3 or more takes it
        assert cnt["the next millisecond"] == 0 and row["the next millisecond"][0] == np.complex64(0.5 + 0.5j)
        for offset in (0, 1):
            flat = np.full(offset + x.size + 3, POISON, dtype=np.complex64)
            flat[offset:offset + x.size] = x
            for in_place in (False, True):
                out, _, counts = _blank(eng, flat, offset, 1, 0, len(names), n, b, in_place)
                got = out[offset:offset + x.size]
                for m, name in enumerate(names):
                    assert counts[0, m] == want_counts[m], (name, guard, offset, in_place, int(counts[0, m]), int(want_counts[m]))
                    assert np.array_equal(_bits(got[m * n:(m + 1) * n]), _bits(row[name])), (name, guard, offset, in_place)
                assert np.isnan(out[:offset].real).all() and np.isnan(out[offset + x.size:].real).all()


def test_no_hit_in_place_writes_nothing(eng):
    """Noise far below the threshold between poisoned neighbours: the buffer's bits are the input's, every count is 0."""
    n, n_ms = 4092, 2
    rng = np.random.default_rng(4)
    for offset in (2, 3):
        flat = np.full(offset + n_ms * n + 4, POISON, dtype=np.complex64)
        flat[offset:offset + n_ms * n] = (rng.standard_normal(n_ms * n) + 1j * rng.standard_normal(n_ms * n)).astype(np.complex64)
        out, _, counts = _blank(eng, flat, offset, 1, 0, n_ms, n, Blanker(0.0, 0.0, 100.0, 64), True)
        assert np.array_equal(_bits(out), _bits(flat)) and not counts.any()


def test_a_centre_like_an_offset_binary_recordings(eng):
    """uint8-like words about 127.4: the decision is taken about the centre and blanked samples become exactly the centre."""
    n, n_ms = 2046, 2
    rng = np.random.default_rng(127)
    x = np.clip(np.rint(127.4 + 6.0 * rng.standard_normal(n_ms * n)), 0, 255) + 1j * np.clip(np.rint(127.4 + 6.0 * rng.standard_normal(n_ms * n)), 0, 255)
    x[[5, 900, n + 2000]] = 255.0 + 0.0j
    x = x.astype(np.complex64)
    b = Blanker(127.4, 127.4, 40.0, 4)
    want, want_counts = model.blank(x, n, _m(b))
    assert want_counts.tolist() == [18, 9] and want[900] == np.complex64(complex(np.float32(127.4), np.float32(127.4)))
    for in_place in (False, True):
        out, _, counts = _blank(eng, x, 0, 1, 0, n_ms, n, b, in_place)
        assert np.array_equal(_bits(out), _bits(want)) and counts[0].tolist() == want_counts.tolist()
    assert not _blank(eng, x, 0, 1, 0, n_ms, n, Blanker(0.0, 0.0, 400.0, 4), True)[2].any()     # about 0 nothing reaches 400


def test_the_same_bits_for_every_call_shape(eng):
    """3 streams x 4 ms in one call against: stream by stream, millisecond by millisecond, a sub-window, rows moved onto 16 bytes,
    and 1 and 8 workgroups per CU."""
    n, n_ms = 2046, 4
    stride = n_ms * n + 3
    flat = _pulsed(1 + 3 * stride, 99)
    blankers = [Blanker(0.0, 0.0, 4.0, 4), Blanker(0.1, 0.2, 3.0, 64), Blanker(0.0, 0.0, 5.0, 0)]
    got, _, got_counts = _blank(eng, flat, 1, 3, stride, n_ms, n, blankers, False)
    assert got_counts.min() > 0
    for s in range(3):
        a = 1 + s * stride
        one, _, c = _blank(eng, flat, a, 1, 0, n_ms, n, blankers[s], True)
        assert _same(one[a:a + n_ms * n], got[a:a + n_ms * n]) and _same(c[0], got_counts[s]), s
        for m in range(n_ms):
            ms, _, c = _blank(eng, flat, a + m * n, 1, 0, 1, n, blankers[s], False)
            assert _same(ms[a + m * n:a + (m + 1) * n], got[a + m * n:a + (m + 1) * n]) and c[0, 0] == got_counts[s, m], (s, m)
        sub, _, c = _blank(eng, flat, a + n, 1, 0, 2, n, blankers[s], True)
        assert _same(sub[a + n:a + 3 * n], got[a + n:a + 3 * n]) and _same(c[0], got_counts[s, 1:3]), s
        moved = np.ascontiguousarray(flat[a:a + n_ms * n])
        out, _, c = _blank(eng, moved, 0, 1, 0, n_ms, n, blankers[s], True)
        assert _same(out, got[a:a + n_ms * n]) and _same(c[0], got_counts[s]), s
    try:
        for per_cu in (1, 8):
            eng.debug_set("widen_wg_per_cu", per_cu)
            out, _, c = _blank(eng, flat, 1, 3, stride, n_ms, n, blankers, False)
            assert _same(out, got) and _same(c, got_counts), per_cu
    finally:
        eng.debug_set("widen_wg_per_cu", 2)
    # more streams than one launch carries
    many = np.tile(flat[1:1 + n], 11)
    out, _, c = _blank(eng, many, 0, 11, n, 1, n, [Blanker(0.0, 0.0, 3.0 + 0.25 * s, s) for s in range(11)], True)
    for s in range(11):
        w, wc = model.blank(many[s * n:(s + 1) * n], n, model.Blanker(0.0, 0.0, 3.0 + 0.25 * s, s))
        assert np.array_equal(_bits(out[s * n:(s + 1) * n]), _bits(w)) and c[s, 0] == wc[0], s


def test_blank_arguments_are_checked_before_anything_is_launched(eng):
    d = eng.alloc(1 << 16)
    p, n = d.ptr.value, 2046
    ok = dict(inp=p, out=p, ns=1, stride=n, n_ms=1, n=n, b=Blanker(0.0, 0.0, 3.0, 4))
    cases = {"in NULL": dict(inp=0), "out NULL": dict(out=0), "n_streams 0": dict(ns=0), "n_ms < 0": dict(n_ms=-1), "N 0": dict(n=0),
             "N too large": dict(n=65537), "stride": dict(ns=2, stride=n - 1), "centre inf": dict(b=Blanker(np.inf, 0.0, 3.0, 4)),
             "centre nan": dict(b=Blanker(0.0, np.nan, 3.0, 4)), "threshold 0": dict(b=Blanker(0.0, 0.0, 0.0, 4)),
             "threshold < 0": dict(b=Blanker(0.0, 0.0, -3.0, 4)), "threshold inf": dict(b=Blanker(0.0, 0.0, np.inf, 4)),
             "threshold nan": dict(b=Blanker(0.0, 0.0, np.nan, 4)), "guard -1": dict(b=Blanker(0.0, 0.0, 3.0, -1)), "guard 65": dict(b=Blanker(0.0, 0.0, 3.0, 65))}
    for what, change in cases.items():
        a = dict(ok, **change)
        with pytest.raises(_lib.GypsumHipError, match="gyp_blank_iq_dev") as e:
            eng.blank_iq_dev(a["inp"], a["out"], a["ns"], a["stride"], a["n_ms"], a["n"], a["b"])
        assert e.value.code == BAD, what
    assert eng.lib.gyp_blank_iq_dev(eng.ctx, p, p, 1, n, 1, n, None, None) == BAD
    eng.blank_iq_dev(p, p, 1, n, 0, n, ok["b"])                                   # nothing to do
    for what, args in {"iq NULL": (0, 1, n, n, None, p), "hist NULL": (p, 1, n, n, None, 0), "n_streams 0": (p, 0, n, n, None, p),
                       "n_samples 0": (p, 1, n, 0, None, p), "stride": (p, 2, n - 1, n, None, p), "centre inf": (p, 1, n, n, [np.inf, 0.0], p),
                       "centre nan": (p, 1, n, n, [0.0, np.nan], p)}.items():
        with pytest.raises(_lib.GypsumHipError, match="gyp_iq_power_hist_dev") as e:
            eng.power_hist_dev(*args)
        assert e.value.code == BAD, what
    eng.sync()
    d.free()


# ---------------------------------------------------------------------------------------------------- histogram
def _hist(eng, flat, offset, n_streams, stride, n_samples, centers, d_out=None):
    d_iq = eng.alloc(flat.nbytes).upload(flat)
    own = d_out is None
    if own:
        d_out = eng.alloc(4 * model.BINS * n_streams + 4).upload(np.full(model.BINS * n_streams + 1, 0xABCD1234, dtype=np.uint32))
    eng.power_hist_dev(d_iq.ptr.value + 8 * offset, n_streams, stride, n_samples, centers, d_out.ptr.value)
    out = d_out.download(np.uint32, model.BINS * n_streams + 1)
    assert out[-1] == 0xABCD1234
    d_iq.free()
    if own:
        d_out.free()
    return out[:-1].reshape(n_streams, model.BINS)


@pytest.mark.parametrize("n_samples", [1, 2046, 5 * 4092 + 3])
def test_the_histogram_equals_the_models_integers(eng, n_samples):
    """Two streams, rows on 16 bytes and 8 bytes off, with and without centres; zeros, a denormal power, an inf and a NaN among the
    samples; split calls summed on the host; a second call into the same buffer overwrites."""
    stride = n_samples + 3
    for offset in (0, 1):
        flat = _pulsed(offset + 2 * stride, n_samples + offset)
        rows = [slice(offset + s * stride, offset + s * stride + n_samples) for s in range(2)]
        if n_samples > 100:
            flat[rows[0]][[3, 4, 50, 51, 60]] = [0.0, 0.0, 7e-20, complex(np.inf, 1.0), complex(np.nan, 1.0)]
            flat[rows[1]][[0, n_samples - 1]] = [complex(0.0, -np.inf), 7e-20j]
        for centers in (None, [0.25 + 0.5j, -1.0 + 0j]):
            c = [0j, 0j] if centers is None else centers
            want = np.stack([model.hist(flat[rows[s]], c[s]) for s in range(2)])
            assert want.sum(axis=1).tolist() == [n_samples] * 2
            got = _hist(eng, flat, offset, 2, stride, n_samples, None if centers is None else np.array([[v.real, v.imag] for v in c]))
            assert np.array_equal(got, want), (n_samples, offset, centers, np.flatnonzero(got != want)[:8])
            if n_samples > 100 and centers is None:
                assert want[0, 0] == 2 and want[0, 2040] == 1 and want[0, 2044] == 1 and want[1, 2040] == 1
                assert 0 < np.flatnonzero(want[0])[1] < 8                               # the denormal power
        if n_samples > 100:
            cut = n_samples // 3 + 1
            parts = _hist(eng, flat, offset, 2, stride, cut, None) + _hist(eng, flat, offset + cut, 2, stride, n_samples - cut, None)
            whole = np.stack([model.hist(flat[rows[s]]) for s in range(2)])
            assert np.array_equal(parts, whole), (n_samples, offset)
            d_out = eng.alloc(4 * model.BINS * 2 + 4).upload(np.full(model.BINS * 2 + 1, 0xABCD1234, dtype=np.uint32))
            _hist(eng, flat, offset, 2, stride, n_samples, None, d_out)
            again = _hist(eng, flat, offset, 2, stride, n_samples, None, d_out)
            d_out.free()
            assert np.array_equal(again, whole)
    try:
        eng.debug_set("widen_wg_per_cu", 8)
        assert np.array_equal(_hist(eng, flat, 1, 2, stride, n_samples, None), np.stack([model.hist(flat[rows[s]]) for s in range(2)]))
    finally:
        eng.debug_set("widen_wg_per_cu", 2)
    assert np.array_equal(eng.power_hist(flat[rows[0]], 0.25 + 0.5j), model.hist(flat[rows[0]], 0.25 + 0.5j))


# ---------------------------------------------------------------------------------------------------- ingest
def _download(eng, dev, count):
    buf = np.empty(count, dtype=np.complex64)
    eng._check(eng.lib.gyp_memcpy_d2h(eng.ctx, _lib.ptr(buf), _lib.C.c_void_p(dev), buf.nbytes))
    return buf


def _drain(eng, ing, blanked=None):
    """(first milliseconds, samples); with `blanked` a list, last_blanked() of every block is appended to it."""
    got, firsts = [], []
    while (blk := ing.next_device_block()) is not None:
        f, count, dev = blk
        if blanked is not None:
            blanked.append(ing.last_blanked())
        got.append(_download(eng, dev, count * ing.n))
        firsts.append(f)
    return firsts, (np.concatenate(got) if got else np.empty(0, np.complex64))


N_FILE_MS = 12


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    """The pulsed scene over 12 ms as a float32 recording and as offset-binary uint8 words."""
    d = tmp_path_factory.mktemp("blank")
    x, clean = model.scene(N_FILE_MS)
    _, u8, q = notch_model.scene_words(x)
    np.concatenate([x, np.zeros(1, np.complex64)]).view(np.float32).tofile(d / "pulsed.f32")
    np.concatenate([u8, np.full(2, 128, np.uint8)]).tofile(d / "pulsed.u8")
    return {"x": x, "clean": clean, "q": q, np.float32: d / "pulsed.f32", np.uint8: d / "pulsed.u8"}


FIXED = {np.float32: Blanker(0.0, 0.0, 0.26, 4), np.uint8: Blanker(127.4, 128.0, 9.0, 7)}


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
@pytest.mark.parametrize("block_ms", [1, 7])
def test_a_handles_blocks_are_blanked_as_one_call_would(eng, scene_files, block_ms, dtype):
    """Block by block through a float32 and a uint8 handle, from the start and after a seek: the bits of one gyp_blank_iq_dev call
    over the handle's plain output, which are the model's; host blocks are refused while the blanker is on; None switches it off."""
    n, b = model.SCENE_N, FIXED[dtype]
    ing = IqFileIngest(scene_files[dtype], model.SCENE_FS, dtype, block_ms=block_ms, depth=3, engine=eng)
    try:
        assert ing.total_ms == N_FILE_MS and ing.blanker is None
        _, plain = _drain(eng, ing)
        want, counts = eng.blank_iq(plain, n, b)
        model_want, model_counts = model.blank(plain, n, _m(b))
        assert np.array_equal(_bits(want), _bits(model_want)) and np.array_equal(counts, model_counts)
        assert 0.08 * plain.size < counts.sum() < 0.2 * plain.size
        ing.set_blanker(b)
        assert ing.blanker == Blanker.from_record(b.record())
        for at in (0, 5):
            ing.seek(at)
            firsts, got = _drain(eng, ing)
            assert firsts == list(range(at, N_FILE_MS, block_ms)) and np.array_equal(_bits(got), _bits(want[at * n:])), (block_ms, at)
        with pytest.raises(_lib.GypsumHipError, match="gyp_ingest_next_host") as e:
            ing.next_host_block()
        assert e.value.code == BAD
        with pytest.raises(_lib.GypsumHipError, match="gyp_ingest_set_blanker"):
            ing.set_blanker(Blanker(0.0, 0.0, 1.0, 65))
        assert ing.blanker == Blanker.from_record(b.record())
        ing.set_blanker(None)
        ing.seek(0)
        assert np.array_equal(_bits(_drain(eng, ing)[1]), _bits(plain)) and ing.blanker is None
        ing.seek(0)
        assert ing.next_host_block() is not None
    finally:
        ing.close()


@pytest.mark.parametrize("block_ms", [1, 7])
def test_last_blanked_counts_each_block_as_the_model_does(eng, scene_files, block_ms):
    n, b = model.SCENE_N, FIXED[np.float32]
    _, want = model.blank(scene_files["x"], n, _m(b))
    ing = IqFileIngest(scene_files[np.float32], model.SCENE_FS, np.float32, block_ms=block_ms, depth=3, engine=eng)
    try:
        assert ing.last_blanked().size == 0                                     # no block yet
        off = []
        firsts, _ = _drain(eng, ing, off)
        assert [len(c) for c in off] == [min(block_ms, N_FILE_MS - f) for f in firsts] and not np.concatenate(off).any()
        ing.set_blanker(b)
        assert ing.last_blanked().size == 0                                     # set_blanker reads again from the cursor
        ing.seek(0)
        on = []
        firsts, _ = _drain(eng, ing, on)
        for f, c in zip(firsts, on):
            assert c.tolist() == want[f:f + block_ms].tolist(), f
        assert np.concatenate(on).sum() == want.sum() > 0
    finally:
        ing.close()


def test_the_chain_is_blanker_then_notches_then_level(eng, scene_files):
    """With a blanker, one notch and a level installed a handle's output is the level applied to the notch of the model-blanked
    samples: bit for bit against the device's stand-alone notch and level on the model's output (their own tests tie those to
    their float64 models), and against notch_model.notch in float64 within the notch test's derived bound."""
    n, fs, b = model.SCENE_N, model.SCENE_FS, FIXED[np.float32]
    tone, level = 217_300, IqLevel(0.015625, -0.03125, 3.0)
    blanked, _ = model.blank(scene_files["x"], n, _m(b))
    ing = IqFileIngest(scene_files[np.float32], fs, np.float32, block_ms=5, depth=3, engine=eng)
    try:
        ing.set_level(level)
        ing.set_notches([tone])
        ing.set_blanker(b)
        assert (ing.blanker, ing.notches, ing.level) == (Blanker.from_record(b.record()), [tone], level)
        _, got = _drain(eng, ing)
        notched = eng.notch_iq(blanked, fs, n, [tone])
        assert np.array_equal(_bits(got), _bits(eng.condition_iq(notched, level)))
        other_order = eng.blank_iq(eng.notch_iq(scene_files["x"], fs, n, [tone]), n, b)[0]
        assert not np.array_equal(_bits(notched), _bits(other_order))                # the order is observable on this scene
        ing.set_level(None)
        ing.seek(0)
        _, got = _drain(eng, ing)
        want, amps = notch_model.notch(blanked, fs, n, [tone])
        bound = np.repeat(2.0 ** -20 * np.abs(amps).sum(axis=1), n) + 2.0 ** -23 * np.abs(blanked.astype(np.complex128))
        g = got.astype(np.complex128)
        assert (np.maximum(np.abs(g.real - want.real), np.abs(g.imag - want.imag)) <= bound).all()
    finally:
        ing.close()


def test_find_pulses_does_not_depend_on_the_blocks_and_leaves_the_cursor(eng, scene_files):
    """The float32 handle: centre 0 (remove_dc off) and the model's blanker of the first 10 ms, the same for block_ms 1, 7 and 100;
    the uint8 handle: a centre near 128 -- the mean, as gyp_iq_level_from_stats takes it."""
    n, fs = model.SCENE_N, model.SCENE_FS
    x = scene_files["x"]
    want, median, t = model.from_hist(model.hist(x[:10 * n]), 0j, 16.0, 4)
    results = []
    for block_ms in (1, 7, 100):
        ing = IqFileIngest(scene_files[np.float32], fs, np.float32, block_ms=block_ms, depth=3, engine=eng)
        try:
            first = ing.next_device_block()[0]
            b, measured = ing.find_pulses(first_ms=0, n_ms=10, remove_dc=False, install=False)
            assert ing.blanker is None
            assert (b.center_re, b.center_im, b.threshold, b.guard) == tuple(want) and measured == {"median": median, "threshold": t}
            nxt = ing.next_device_block()                               # the cursor is where it was
            assert first == 0 and (nxt is None if block_ms >= N_FILE_MS else nxt[0] == block_ms)
            with_dc, _ = ing.find_pulses(first_ms=1, n_ms=10, guard=9)
            assert ing.blanker == with_dc and with_dc.guard == 9
            mean = x[n:11 * n].astype(np.complex128).mean()
            assert abs(complex(with_dc.center_re, with_dc.center_im) - mean) <= 1e-6 * max(1.0, abs(mean)) + 2.0 ** -24 * abs(mean)
            results.append((b, with_dc))
            for first_ms, n_ms in ((-1, 5), (8, 5), (0, 0), (0, 1001)):
                with pytest.raises(_lib.GypsumHipError, match="gyp_ingest_find_pulses") as e:
                    ing.find_pulses(first_ms=first_ms, n_ms=n_ms)
                assert e.value.code == BAD
            for kw in (dict(threshold_over_median=0.0), dict(threshold_over_median=np.inf), dict(guard=-1), dict(guard=65)):
                with pytest.raises(_lib.GypsumHipError, match="gyp_ingest_find_pulses"):
                    ing.find_pulses(**kw)
            assert ing.blanker == with_dc                               # a refused call leaves the blanker alone
        finally:
            ing.close()
    assert results[0] == results[1] == results[2]
    ing = IqFileIngest(scene_files[np.uint8], fs, np.uint8, block_ms=7, depth=3, engine=eng)
    try:
        b, measured = ing.find_pulses(first_ms=0, n_ms=10)
        twin = IqFileIngest(scene_files[np.uint8], fs, np.uint8, block_ms=12, depth=3, engine=eng)
        _, plain = _drain(eng, twin)
        twin.close()
        stats = eng.iq_stats(plain[:10 * n], n)
        m_re, m_im = stats["sum_re"].sum() / (10.0 * n), stats["sum_im"].sum() / (10.0 * n)
        assert (b.center_re, b.center_im) == (float(np.float32(m_re)), float(np.float32(m_im))) and abs(b.center_re - 128.0) < 0.5
        want_u8, _, _ = model.from_hist(model.hist(plain[:10 * n], complex(b.center_re, b.center_im)), complex(b.center_re, b.center_im), 16.0, 4)
        assert (b.center_re, b.center_im, b.threshold, b.guard) == tuple(want_u8)
    finally:
        ing.close()


def test_calibrate_after_find_pulses_measures_the_blanked_stream(eng, scene_files):
    n, fs = model.SCENE_N, model.SCENE_FS
    ing = IqFileIngest(scene_files[np.float32], fs, np.float32, block_ms=7, depth=3, engine=eng)
    try:
        pulsed_level, _ = ing.calibrate(first_ms=0, n_ms=10)
        ing.set_level(None)
        b, _ = ing.find_pulses(first_ms=0, n_ms=10, remove_dc=False)
        blanked, _ = model.blank(scene_files["x"], n, _m(b))
        want, _ = level_from_stats(eng.iq_stats(blanked[:10 * n], n), n, default_target_rms(n))
        level, measured = ing.calibrate(first_ms=0, n_ms=10)
        assert level == want and ing.level == level and ing.blanker == b
        assert level.gain > 2.0 * pulsed_level.gain                   # 10 % of the samples at +30 dB: the pulsed RMS was 10 dB off
        ing.seek(0)
        assert np.array_equal(_bits(_drain(eng, ing)[1]), _bits(eng.condition_iq(blanked, level)))
        # find_tones, too, searches the blanked output: nothing to find here, and it says so without disturbing the rest
        assert ing.find_tones(first_ms=0, n_ms=10) == [] and ing.blanker == b and ing.level == level
    finally:
        ing.close()


def test_a_failed_find_pulses_restores_blanker_notches_level_and_cursor(eng, tmp_path):
    """A range beyond total_ms is refused at once; a NaN word in millisecond 6 makes the range's mean not finite after the conditioning
    has been put aside.  After each the handle has what it had, and its blocks are those of a twin nothing was asked of."""
    fs, n, n_ms = model.SCENE_FS, model.SCENE_N, 12
    words = np.random.default_rng(6).standard_normal((n_ms * n + 1) * 2).astype(np.float32)
    words[2 * (6 * n + 100)] = np.nan
    path = tmp_path / "nan.f32"
    words.tofile(path)
    level, tones, b = IqLevel(0.25, -0.5, 2.0), [100_000, -300_000], Blanker(0.0, 0.0, 2.5, 3)
    subject, twin = (IqFileIngest(path, fs, np.float32, block_ms=2, depth=3, engine=eng) for _ in range(2))

    def block(ing):
        f, count, dev = ing.next_device_block()
        return f, count, _download(eng, dev, count * n).view(np.uint32)

    try:
        for ing in (subject, twin):
            ing.set_level(level)
            ing.set_notches(tones)
            ing.set_blanker(b)
        first = [block(ing) for ing in (subject, twin)]
        assert first[0][:2] == first[1][:2] == (0, 2) and _same(first[0][2], first[1][2])
        for kw, text in ((dict(first_ms=8, n_ms=5), "total_ms"), (dict(first_ms=4, n_ms=4), "mean is not finite")):
            with pytest.raises(_lib.GypsumHipError, match=text) as e:
                subject.find_pulses(**kw)
            assert e.value.code == BAD
            assert (subject.blanker, subject.notches, subject.level) == (b, tones, level)
        found, _ = subject.find_pulses(first_ms=0, n_ms=4, install=False)             # no NaN there: returns normally
        assert found.guard == 4 and (subject.blanker, subject.notches, subject.level) == (b, tones, level)
        for want_first in range(2, n_ms, 2):
            a, c = block(subject), block(twin)
            assert a[:2] == c[:2] == (want_first, 2) and _same(a[2], c[2]), want_first
        assert subject.next_device_block() is None and twin.next_device_block() is None
    finally:
        subject.close()
        twin.close()


def test_the_provider_blanks_first_then_finds_tones_then_calibrates(eng, tmp_path):
    """An RTL-SDR style recording: uint8 at 2.048 Msps with bursts that saturate the converter, resampled to 2.046 Msps.  The
    provider that measures equals the one given the blanker and the level it reports; its default guard is half the filter's taps."""
    rng = np.random.default_rng(2048)
    count = 12 * 2048 + 1
    x = 1.5 * (rng.standard_normal(count) + 1j * rng.standard_normal(count)) + model.pulses(count, 1.5, 7, db=30.0)
    words = np.empty(2 * count)
    words[0::2], words[1::2] = x.real + 127.4, x.imag + 127.4
    path = tmp_path / "rtl.u8"
    np.clip(np.rint(words), 0, 255).astype(np.uint8).tofile(path)
    kw = dict(sample_component_data_type=np.uint8, block_ms=5, engine=eng)
    prov = AntennaSampleProviderResampled(path, 2_048_000, find_pulses=True, find_tones=True, calibrate=dict(first_ms=0, n_ms=8), **kw)
    ing = IqFileIngest(path, 2_046_000, np.uint8, block_ms=5, depth=3, engine=eng, resample_from_hz=2_048_000)
    try:
        assert prov.blanker.guard == 16 and abs(prov.blanker.center_re - 127.4) < 0.5 and prov.pulses["threshold"] == pytest.approx(prov.blanker.threshold)
        b, _ = ing.find_pulses(guard=16)
        assert b == prov.blanker and ing.find_tones() == prov.tones
        level, _ = ing.calibrate(first_ms=0, n_ms=8)
        assert prov.level == level
        unblanked = IqFileIngest(path, 2_046_000, np.uint8, block_ms=5, depth=3, engine=eng, resample_from_hz=2_048_000)
        pulsed_level, _ = unblanked.calibrate(first_ms=0, n_ms=8)
        unblanked.close()
        assert level.gain > 2.0 * pulsed_level.gain
        got = prov.get_block(12).samples
        assert np.array_equal(_bits(got), _bits(_drain(eng, ing)[1]))
        fixed = AntennaSampleProviderResampled(path, 2_048_000, blank=prov.blanker, level=level, **kw)
        assert np.array_equal(_bits(fixed.get_block(12).samples), _bits(got))
        fixed.close()
        with pytest.raises(ValueError, match="exclude"):
            AntennaSampleProviderResampled(path, 2_048_000, blank=b, find_pulses=True, **kw)
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


def test_a_pulsed_recording_is_acquired_and_tracked_once_its_pulses_are_blanked(eng, tmp_path):
    """The gated scene as a float32 recording.  Un-blanked the detector misses planted satellites, as the gate says
    (tests/test_blank_host.py); after find_pulses the device's acquisition of the blanked block equals the oracle's acquisition of the
    model-blanked stream (Doppler and code phase exact, strength within test_gpu_parity's tolerance, above 3), and 300 ms of tracking
    of the four channels give the oracle's pseudosymbols.  The M2M4 C/N0 per channel is printed, not asserted."""
    fs, n, n_track = model.SCENE_FS, model.SCENE_N, 300
    x, _ = model.scene(n_track)
    path = tmp_path / "pulsed.f32"
    np.concatenate([x, np.zeros(1, np.complex64)]).view(np.float32).tofile(path)
    sats = list(model.SCENE_SATS)
    ing = IqFileIngest(path, fs, np.float32, block_ms=10, depth=3, engine=eng)
    try:
        f, n_ms, dev = ing.next_device_block()
        assert (f, n_ms) == (0, 10)
        raw = _acquire(eng, dev, 10, n, sats)
        missed = [sv for r, sv in zip(raw, sats) if int(r["code_phase"]) != model.SCENE_SATS[sv][0] or float(r["strength"]) <= 3.0]
        print("un-blanked: missed", missed, [(int(r["doppler_hz"]), int(r["code_phase"]), round(float(r["strength"]), 2)) for r in raw])
        assert missed
        b, measured = ing.find_pulses(first_ms=0, n_ms=10)
        print("blanker", b, measured)
        ing.seek(0)
        f, n_ms, dev = ing.next_device_block()
        got = _acquire(eng, dev, 10, n, sats)
        share = ing.last_blanked().sum() / (10.0 * n)
        assert 0.10 <= share <= 0.14
        ing2 = IqFileIngest(path, fs, np.float32, block_ms=n_track, depth=3, engine=eng)
        ing2.set_blanker(b)
        _, blanked = _drain(eng, ing2)
        ing2.close()
    finally:
        ing.close()
    want_stream, _ = model.blank(x, n, _m(b))
    assert np.array_equal(_bits(blanked), _bits(want_stream))
    want_stream = want_stream.astype(np.complex128)
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
    rec = bank.track_block(blanked, 1, n_track, [a for a, _ in times])
    d_rec = eng.alloc(rec.nbytes).upload(rec)                   # for information: the C/N0 the blanked stream tracks at
    d_sums = eng.alloc(len(sats) * SUMS_DTYPE.itemsize)
    bank.quality_dev(d_rec.ptr.value, n_track, n_track, d_sums.ptr.value)
    quality = from_sums(d_sums.download(SUMS_DTYPE, len(sats)))
    print("M2M4 C/N0 per channel (dB-Hz):", [round(float(q["cn0_m2m4_dbhz"]), 2) for q in quality])
    d_rec.free()
    d_sums.free()
    bank.close()
    for i, sv in enumerate(sats):
        trk = orc.Tracker(orc.TrackingState(float(inits[i]["doppler_hz"]), float(inits[i]["carrier_phase"]), int(inits[i]["code_phase"])),
                          orc.prn_as_complex(chips[sv - 1], n), fs, n)
        rows = [trk.process_samples(want_stream[j * n:(j + 1) * n], st, en) for j, (st, en) in enumerate(times)]
        assert [int(v) for v in rec[i]["pseudosymbol"]] == [r.pseudosymbol for r in rows], sv
        assert [int(v) for v in rec[i]["status"]] == [0] * n_track
