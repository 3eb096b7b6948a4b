"""Narrowband and swept interference on the device (gyp_excise_iq_dev, gyp_iq_spectrum_hist_dev, gyp_ingest_set_excisor /
_find_excisor / _last_excised) against tests/excise_model.py: untouched samples bit for bit, decisions on every frame whose bins
stand clear of the threshold, values within a tolerance taken from a float32 restatement of the model, the histogram within what
the same tolerance allows at every bin edge, the same bits for every call shape and grid size, the ingest handle's chain
producer -> blanker -> excisor -> notches -> level, and two scenes whose satellites the detector misses under a 40 dB FM or swept
jammer and finds once the excisor is found and installed."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import excise_model as model
import notch_model
from gypsum_amd import _lib
from gypsum_amd.antenna_sample_provider import AntennaSampleProviderResampled
from gypsum_amd.blanker import Blanker
from gypsum_amd.engine import GypsumEngine
from gypsum_amd.excisor import Excisor, n_frames
from gypsum_amd.ingest import IqFileIngest
from gypsum_amd.level import IqLevel

pytestmark = pytest.mark.gpu

BAD = _lib.GYP_E_BAD_ARG
SHAPES = [(100, 2), (128, 2), (129, 2), (255, 2), (256, 2), (257, 2), (1023, 3), (2046, 3), (4092, 2), (49104, 1)]
GUARDS = (0, 1, 8)
# The tolerances are 8 x what model.excise32 (numpy's single-precision transform) differs from the float64 model by on these very
# inputs (every shape, alignment and guard below; `python tests/test_gpu_excise.py` prints the figures), normalised as the checks
# are: a spectrum's error over the frame's ||w x_f||_2, a sample's over the larger norm of its two frames.
MEASURED_X, MEASURED_Y = 5.32e-7, 3.19e-8
TOL_X, TOL_Y = 8 * MEASURED_X, 8 * MEASURED_Y
POISON = np.complex64(complex(np.nan, np.nan))


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


def _m(e: Excisor) -> model.Excisor:
    return model.Excisor(e.threshold, e.guard)


def _jammed(n, n_ms, seed, quiet_first_ms=False):
    """Unit noise per component, a tone 30 dB above it over [0.15, 0.45) of the row and a sweep 30 dB above it over [0.6, 0.8):
    some frames have hits and some have none; with quiet_first_ms the first millisecond is noise alone."""
    count = n * n_ms
    rng = np.random.default_rng(seed)
    i = np.arange(count, dtype=np.float64)
    x = rng.standard_normal(count) + 1j * rng.standard_normal(count)
    amp = 10.0 ** (30.0 / 20.0)
    tone = amp * np.exp(2j * np.pi * 0.1037 * i)
    f = -0.3 + 0.5 * i / count
    sweep = amp * np.exp(2j * np.pi * np.cumsum(f))
    on_t = (i >= 0.15 * count) & (i < 0.45 * count)
    on_s = (i >= 0.6 * count) & (i < 0.8 * count)
    if quiet_first_ms:
        on_t &= i >= n
        on_s &= i >= n
    return (x + tone * on_t + sweep * on_s).astype(np.complex64)


THRESHOLD = (60.0, 45.0)      # per stream; windowed unit noise has a mean bin power of 192: 19 and 10.5 times it


@functools.lru_cache(maxsize=None)
def _case(n, n_ms, offset):
    """(flat buffer with NaN between the rows, stride, the two rows' slices): two streams; a NaN sample in stream 0."""
    stride = n_ms * n + (2 if offset == 0 else 3)            # rows on 16 bytes stay there; the others alternate
    flat = np.full(offset + 2 * stride + 5, POISON, dtype=np.complex64)
    rows = [slice(offset + s * stride, offset + s * stride + n_ms * n) for s in range(2)]
    flat[rows[0]] = _jammed(n, n_ms, 1000 + n)
    flat[rows[1]] = _jammed(n, n_ms, 2000 + n, quiet_first_ms=True)
    flat[rows[0]][n_ms * n - 7] = np.nan                     # a NaN sample in stream 0, in a millisecond that has hits elsewhere
    flat.setflags(write=False)
    return flat, stride, rows


@functools.lru_cache(maxsize=None)
def _reference(n, n_ms, offset, stream):
    """Per millisecond of one stream of _case: the float64 spectra [n_ms, nf, 256], each frame's ||w x_f||_2 [n_ms, nf] and whether
    the frame holds a NaN."""
    flat, _, rows = _case(n, n_ms, offset)
    row = flat[rows[stream]]
    X = np.stack([model.spectra(row[m * n:(m + 1) * n]) for m in range(n_ms)])
    fr = np.stack([model.frames(row[m * n:(m + 1) * n].astype(np.complex128)) for m in range(n_ms)]) * model.window().astype(np.float64)
    with np.errstate(invalid="ignore"):
        norm = np.sqrt((np.abs(fr) ** 2).sum(axis=-1))
    return X, norm, np.isnan(norm)


def _decisive(X, norm, has_nan, t2):
    """Frames every bin of which stands clear of the threshold by more than a transform error of TOL_X ||w x_f||_2 can move its
    power; a frame with a NaN is decisive: nothing in it is a hit, in any arithmetic."""
    with np.errstate(invalid="ignore"):
        eps = TOL_X * norm[..., None]
        p = X.real ** 2 + X.imag ** 2
        clear = np.abs(p - float(t2)) > 2.0 * np.abs(X) * eps + eps ** 2
    return clear.all(axis=-1) | has_nan


def _t2(e):
    return np.float32(e.threshold) * np.float32(e.threshold)


def _excise(eng, flat, offset, n_streams, stride, n_ms, n, excisors, in_place, want_masks=True):
    """(output buffer, input buffer, counts[n_streams, n_ms], masks[n_streams, n_ms, nf, 4]) after gyp_excise_iq_dev, whole buffers
    downloaded; out of place the output starts as NaN; counts start as -1 and masks as all ones, with a word behind each that must stay."""
    assert offset + (n_streams - 1) * stride + n_ms * n <= flat.size      # the kernel touches nothing else
    nf = n_frames(n)
    d_in = eng.alloc(flat.nbytes).upload(flat)
    d_out = d_in if in_place else eng.alloc(flat.nbytes).upload(np.full(flat.size, POISON, dtype=np.complex64))
    d_cnt = eng.alloc(4 * n_streams * n_ms + 4).upload(np.full(n_streams * n_ms + 1, -1, dtype=np.int32))
    n_words = n_streams * n_ms * nf * 4
    d_msk = eng.alloc(8 * n_words + 8).upload(np.full(n_words + 1, ~np.uint64(0), dtype=np.uint64))
    eng.excise_iq_dev(d_in.ptr.value + 8 * offset, d_out.ptr.value + 8 * offset, n_streams, stride, n_ms, n, excisors, d_cnt.ptr.value,
                      d_msk.ptr.value if want_masks else 0)
    out, src = d_out.download(np.complex64, flat.size), d_in.download(np.complex64, flat.size)
    cnt, msk = d_cnt.download(np.int32, n_streams * n_ms + 1), d_msk.download(np.uint64, n_words + 1)
    assert cnt[-1] == -1 and msk[-1] == ~np.uint64(0)
    for d in (d_in, d_cnt, d_msk) + (() if in_place else (d_out,)):
        d.free()
    return out, src, cnt[:-1].reshape(n_streams, n_ms), msk[:-1].reshape(n_streams, n_ms, nf, 4)


def _touched(cut, n):
    """[n_ms, n] bool: the samples one of whose two frames excised something, from [n_ms, nf, 256] bool."""
    any_f = cut.any(axis=-1)                                  # [n_ms, nf]
    hop = any_f[:, :-1] | any_f[:, 1:]                        # hop j lies in frames j and j + 1
    return np.repeat(hop, model.HOP, axis=1)[:, :n]


def _sample_norm(norm, n):
    """[n_ms, n]: the larger ||w x_f||_2 of each sample's two frames (a NaN norm does not count)."""
    return np.repeat(np.fmax(norm[:, :-1], norm[:, 1:]), model.HOP, axis=1)[:, :n]


# ---------------------------------------------------------------------------------------------------- samples, masks, counts
@pytest.mark.parametrize("offset", [0, 1], ids=["rows on 16 bytes", "rows 8 bytes off"])
@pytest.mark.parametrize("n,n_ms", SHAPES)
def test_excised_samples_masks_and_counts_against_the_model(eng, n, n_ms, offset):
    """Below one hop, exactly one, one sample over; odd rows that alternate alignment; a last frame of two samples (2046); the
    streamed case (49104: 385 frames).  Two streams with their own excisors, guards 0, 1 and 8, in place and out of place, NaN
    around the rows, one NaN sample in stream 0.  Exact: untouched samples and the buffer around the rows keep their bits, counts
    are the masks' popcounts.  Decisions on decisive frames equal the model's.  Values against the model fed the device's masks."""
    flat, stride, rows = _case(n, n_ms, offset)
    nf = n_frames(n)
    some_hit = some_none = False
    for guard in GUARDS:
        excisors = [Excisor(THRESHOLD[0], guard), Excisor(THRESHOLD[1], guard)]
        decisive, want_cut = [], []
        for s in range(2):
            X, norm, has_nan = _reference(n, n_ms, offset, s)
            d = _decisive(X, norm, has_nan, _t2(excisors[s]))
            assert (~d).sum() <= 0.01 * d.size, (n, s, int((~d).sum()), d.size)     # on the model alone
            decisive.append(d)
            want_cut.append(model.unpack_masks(model.excise(flat[rows[s]], n, _m(excisors[s]))[1]))
        for in_place in (False, True):
            out, src, counts, masks = _excise(eng, flat, offset, 2, stride, n_ms, n, excisors, in_place)
            what = (n, offset, guard, in_place)
            outside = np.ones(flat.size, dtype=bool)
            for s in range(2):
                outside[rows[s]] = False
                cut = model.unpack_masks(masks[s])
                assert cut.shape == (n_ms, nf, 256)
                assert np.array_equal(counts[s], cut.sum(axis=(1, 2))), (what, s)
                assert np.array_equal(cut[decisive[s]], want_cut[s][decisive[s]]), (what, s)
                _, _, has_nan = _reference(n, n_ms, offset, s)
                assert not cut[has_nan].any(), (what, s)
                some_hit |= bool(cut.any(axis=-1).any())
                some_none |= bool((~cut.any(axis=-1)).any())
                touched = _touched(cut, n).reshape(-1)
                got, x = out[rows[s]], flat[rows[s]]
                assert np.array_equal(_bits(got)[~touched], _bits(x)[~touched]), (what, s)
                want, _, _ = model.excise(x, n, _m(excisors[s]), masks=masks[s])
                scale = _sample_norm(_reference(n, n_ms, offset, s)[1], n).reshape(-1)
                with np.errstate(invalid="ignore"):
                    err = np.abs(got.astype(np.complex128) - want.astype(np.complex128)) / scale
                ok = np.isnan(x.real) | (err <= TOL_Y) | ~touched                  # (the NaN sample stays a NaN)
                assert ok.all(), (what, s, float(np.nanmax(err[touched])) if touched.any() else 0.0, TOL_Y)
                if touched.any():
                    print(f"{what} stream {s}: worst sample error {np.nanmax(err[touched]):.3g} of TOL_Y {TOL_Y:.3g}; "
                          f"{int((~decisive[s]).sum())} of {decisive[s].size} frames not decisive")
            if in_place:
                assert np.isnan(out[outside].real).all(), what                     # (the poison between the rows)
            else:
                assert np.isnan(out[outside].real).all() and np.array_equal(_bits(src), _bits(flat)), what
    assert some_hit and some_none


def test_nothing_hit_in_place_writes_nothing_and_out_of_place_copies(eng):
    n, n_ms = 2046, 2
    rng = np.random.default_rng(4)
    for offset in (2, 3):
        flat = np.full(offset + n_ms * n + 4, POISON, dtype=np.complex64)
        flat[offset:offset + n_ms * n] = (rng.standard_normal(n_ms * n) + 1j * rng.standard_normal(n_ms * n)).astype(np.complex64)
        flat[offset + 5] = np.complex64(complex(-0.0, 3.0))
        out, _, counts, masks = _excise(eng, flat, offset, 1, 0, n_ms, n, Excisor(1e4, 8), True)
        assert np.array_equal(_bits(out), _bits(flat)) and not counts.any() and not masks.any()
        out, _, counts, masks = _excise(eng, flat, offset, 1, 0, n_ms, n, Excisor(1e4, 8), False)
        assert np.array_equal(_bits(out[offset:offset + n_ms * n]), _bits(flat[offset:offset + n_ms * n])) and not counts.any()


def test_a_tone_between_two_bins_at_the_rings_seam_takes_its_guard_round_it(eng):
    """Half a bin below 0 Hz: the hits are bins 255 and 0 and a guard of 2 excises 253 .. 2 -- the model's masks, and the tone is
    gone from the samples both of whose frames lie inside the millisecond."""
    n = 512
    i = np.arange(n)
    rng = np.random.default_rng(6)
    x = (0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + np.exp(-2j * np.pi * 0.5 / 256 * i)).astype(np.complex64)
    e = Excisor(20.0, 2)
    want, want_masks, want_counts = model.excise(x, n, _m(e))
    out, _, counts, masks = _excise(eng, x, 0, 1, 0, 1, n, e, True)
    assert np.array_equal(masks[0], want_masks) and counts[0, 0] == want_counts[0]
    cut = model.unpack_masks(masks[0, 0])
    assert cut[1:-1][:, [253, 254, 255, 0, 1, 2]].all() and not cut[:, 8:248].any()
    assert np.abs(out[128:n - 128]).max() < 0.1 and np.abs(out - want).max() < 1e-4


def test_the_same_bits_for_every_call_shape(eng):
    """3 streams x 4 ms in one call against: stream by stream, millisecond by millisecond, a sub-window, rows moved onto 16 bytes,
    1 and 8 workgroups per CU, without masks and counts, and 9 streams (one more than a launch holds) against one at a time."""
    n, n_ms = 2046, 4
    stride = n_ms * n + 3
    flat = np.full(1 + 3 * stride, POISON, dtype=np.complex64)
    for s in range(3):
        flat[1 + s * stride:1 + s * stride + n_ms * n] = _jammed(n, n_ms, 99 + s)
    excisors = [Excisor(60.0, 1), Excisor(45.0, 8), Excisor(80.0, 0)]
    got, _, got_counts, got_masks = _excise(eng, flat, 1, 3, stride, n_ms, n, excisors, False)
    assert got_counts.min(axis=1).min() >= 0 and got_counts.sum(axis=1).min() > 0
    for s in range(3):
        a = 1 + s * stride
        one, _, c, k = _excise(eng, flat, a, 1, 0, n_ms, n, excisors[s], True)
        assert _same(one[a:a + n_ms * n], got[a:a + n_ms * n]) and _same(c[0], got_counts[s]) and _same(k[0], got_masks[s]), s
        for m in range(n_ms):
            ms, _, c, k = _excise(eng, flat, a + m * n, 1, 0, 1, n, excisors[s], False)
            assert _same(ms[a + m * n:a + (m + 1) * n], got[a + m * n:a + (m + 1) * n]) and c[0, 0] == got_counts[s, m], (s, m)
            assert _same(k[0, 0], got_masks[s, m]), (s, m)
        sub, _, c, k = _excise(eng, flat, a + n, 1, 0, 2, n, excisors[s], True)
        assert _same(sub[a + n:a + 3 * n], got[a + n:a + 3 * n]) and _same(c[0], got_counts[s, 1:3]) and _same(k[0], got_masks[s, 1:3]), s
        moved = np.ascontiguousarray(flat[a:a + n_ms * n])
        out, _, c, k = _excise(eng, moved, 0, 1, 0, n_ms, n, excisors[s], True)
        assert _same(out, got[a:a + n_ms * n]) and _same(c[0], got_counts[s]) and _same(k[0], got_masks[s]), s
    try:
        for per_cu in (1, 8):
            eng.debug_set("widen_wg_per_cu", per_cu)
            out, _, c, k = _excise(eng, flat, 1, 3, stride, n_ms, n, excisors, False)
            assert _same(out, got) and _same(c, got_counts) and _same(k, got_masks), per_cu
    finally:
        eng.debug_set("widen_wg_per_cu", 2)
    out, _, _, _ = _excise(eng, flat, 1, 3, stride, n_ms, n, excisors, False, want_masks=False)
    assert _same(out, got)
    # more streams than one launch carries
    many = np.concatenate([_jammed(n, 1, 300 + s) for s in range(9)])
    nine = [Excisor(50.0 + 5.0 * s, s % 9) for s in range(9)]
    out, _, c, k = _excise(eng, many, 0, 9, n, 1, n, nine, True)
    for s in range(9):
        one, _, c1, k1 = _excise(eng, many, s * n, 1, 0, 1, n, nine[s], True)
        assert _same(out[s * n:(s + 1) * n], one[s * n:(s + 1) * n]) and c[s, 0] == c1[0, 0] and _same(k[s], k1[0]), s
    assert c.min() > 0


def test_arguments_are_checked_before_anything_is_launched(eng):
    d = eng.alloc(1 << 16)
    p, n = d.ptr.value, 2046
    ok = dict(inp=p, out=p, ns=1, stride=n, n_ms=1, n=n, e=Excisor(3.0, 1))
    cases = {"in NULL": dict(inp=0), "out NULL": dict(out=0), "n_streams 0": dict(ns=0), "n_ms < 0": dict(n_ms=-1), "N 0": dict(n=0),
             "N too large": dict(n=65537), "stride": dict(ns=2, stride=n - 1), "threshold 0": dict(e=Excisor(0.0, 1)),
             "threshold < 0": dict(e=Excisor(-3.0, 1)), "threshold inf": dict(e=Excisor(np.inf, 1)), "threshold nan": dict(e=Excisor(np.nan, 1)),
             "guard -1": dict(e=Excisor(3.0, -1)), "guard 9": dict(e=Excisor(3.0, 9))}
    for what, change in cases.items():
        a = dict(ok, **change)
        with pytest.raises(_lib.GypsumHipError, match="gyp_excise_iq_dev") as e:
            eng.excise_iq_dev(a["inp"], a["out"], a["ns"], a["stride"], a["n_ms"], a["n"], a["e"])
        assert e.value.code == BAD, what
    rec = Excisor(3.0, 1).record()
    rec["reserved"][0, 1] = 1
    with pytest.raises(_lib.GypsumHipError, match="reserved"):
        eng.excise_iq_dev(p, p, 1, n, 1, n, rec)
    assert eng.lib.gyp_excise_iq_dev(eng.ctx, p, p, 1, n, 1, n, None, None, None) == BAD
    eng.excise_iq_dev(p, p, 1, n, 0, n, ok["e"])                                  # nothing to do
    for what, args in {"iq NULL": (0, 1, n, 1, n, p), "hist NULL": (p, 1, n, 1, n, 0), "n_streams 0": (p, 0, n, 1, n, p),
                       "n_ms 0": (p, 1, n, 0, n, p), "stride": (p, 2, n - 1, 1, n, p), "N 255": (p, 1, 255, 1, 255, p),
                       "N too large": (p, 1, 65537, 1, 65537, p)}.items():
        with pytest.raises(_lib.GypsumHipError, match="gyp_iq_spectrum_hist_dev") as e:
            eng.spectrum_hist_dev(*args)
        assert e.value.code == BAD, what
    eng.sync()
    d.free()


# ---------------------------------------------------------------------------------------------------- histogram
def _hist(eng, flat, offset, n_streams, stride, n_ms, n, d_out=None):
    d_iq = eng.alloc(flat.nbytes).upload(flat)
    own = d_out is None
    if own:
        d_out = eng.alloc(4 * model.BINS * n_streams + 4).upload(np.full(model.BINS * n_streams + 1, 0xABCD1234, dtype=np.uint32))
    eng.spectrum_hist_dev(d_iq.ptr.value + 8 * offset, n_streams, stride, n_ms, n, d_out.ptr.value)
    out = d_out.download(np.uint32, model.BINS * n_streams + 1)
    assert out[-1] == 0xABCD1234
    d_iq.free()
    if own:
        d_out.free()
    return out[:-1].reshape(n_streams, model.BINS)


@pytest.mark.parametrize("offset", [0, 1], ids=["rows on 16 bytes", "rows 8 bytes off"])
@pytest.mark.parametrize("n,n_ms", [s for s in SHAPES if s[0] >= 256])
def test_the_histogram_counts_full_frames_and_follows_the_model_at_every_edge(eng, n, n_ms, offset):
    """The total is 256 x (full frames) x n_ms exactly; at every bin edge the cumulative count differs from the model's by at most
    the number of model powers a transform error of TOL_X ||w x_f||_2 can carry across that edge; the histograms of two parts of a
    stream add up to the whole's bit for bit; a second call into the same buffer overwrites; 8 workgroups per CU count the same."""
    import blank_model
    flat, stride, rows = _case(n, n_ms, offset)
    full = model.full_frames(n)
    got = _hist(eng, flat, offset, 2, stride, n_ms, n)
    assert got.sum(axis=1).tolist() == [256 * len(full) * n_ms] * 2
    edges = blank_model.bin_edges()[:2041]
    for s in range(2):
        X, norm, has_nan = _reference(n, n_ms, offset, s)
        X, eps = X[:, full].reshape(-1), np.repeat(TOL_X * norm[:, full].reshape(-1), 256)
        keep = ~np.isnan(X.real)
        X, eps = X[keep], eps[keep]
        p = X.real ** 2 + X.imag ** 2
        slack = 2.0 * np.abs(X) * eps + eps ** 2
        cum_model = np.searchsorted(np.sort(p), edges, side="left")
        unsure = np.searchsorted(np.sort(p - slack), edges, side="right") - np.searchsorted(np.sort(p + slack), edges, side="left")
        cum_dev = np.concatenate([[0], np.cumsum(got[s].astype(np.int64))])[:2041]
        assert (np.abs(cum_dev - cum_model) <= unsure).all(), (n, offset, s, int(np.abs(cum_dev - cum_model).max()))
        assert got[s, 2040:].sum() == 256 * int(has_nan[:, full].sum())           # a frame with a NaN: 256 NaN powers
        print(f"n {n} stream {s}: {int((cum_dev != cum_model).sum())} of 2041 edges differ, by at most {int(np.abs(cum_dev - cum_model).max())}")
    if n_ms >= 2:
        parts = _hist(eng, flat, offset, 2, stride, 1, n) + _hist(eng, flat, offset + n, 2, stride, n_ms - 1, n)
        assert np.array_equal(parts, got), (n, offset)
    d_out = eng.alloc(4 * model.BINS * 2 + 4).upload(np.full(model.BINS * 2 + 1, 0xABCD1234, dtype=np.uint32))
    _hist(eng, flat, offset, 2, stride, n_ms, n, d_out)
    again = _hist(eng, flat, offset, 2, stride, n_ms, n, d_out)
    d_out.free()
    assert np.array_equal(again, got)
    try:
        eng.debug_set("widen_wg_per_cu", 8)
        assert np.array_equal(_hist(eng, flat, offset, 2, stride, n_ms, n), got)
    finally:
        eng.debug_set("widen_wg_per_cu", 2)
    assert np.array_equal(eng.spectrum_hist(np.ascontiguousarray(flat[rows[1]]), n), got[1])


# ---------------------------------------------------------------------------------------------------- ingest
def _download(eng, dev, count):
    buf = np.empty(count, dtype=np.complex64)
    eng._check(eng.lib.gyp_memcpy_d2h(eng.ctx, _lib.ptr(buf), _lib.C.c_void_p(dev), buf.nbytes))
    return buf


def _drain(eng, ing, excised=None):
    """(first milliseconds, samples); with `excised` a list, last_excised() of every block is appended to it."""
    got, firsts = [], []
    while (blk := ing.next_device_block()) is not None:
        f, count, dev = blk
        if excised is not None:
            excised.append(ing.last_excised())
        got.append(_download(eng, dev, count * ing.n))
        firsts.append(f)
    return firsts, (np.concatenate(got) if got else np.empty(0, np.complex64))


N_FILE_MS = 12


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    """The "fm" and "sweep" scenes over 12 ms as int8 recordings."""
    d = tmp_path_factory.mktemp("excise")
    out = {}
    for kind in ("fm", "sweep"):
        x, clean = model.scene(kind, N_FILE_MS)
        w8, _, q = notch_model.scene_words(x)
        np.concatenate([w8, np.zeros(2, np.int8)]).tofile(d / f"{kind}.i8")
        out[kind] = d / f"{kind}.i8"
    return out


@pytest.fixture(scope="module")
def fm_plain(eng, scene_files):
    """The "fm" handle's un-conditioned output, and the excisor the device finds on its first ten milliseconds."""
    ing = IqFileIngest(scene_files["fm"], model.SCENE_FS, np.int8, block_ms=N_FILE_MS, depth=3, engine=eng)
    try:
        _, plain = _drain(eng, ing)
        e, measured = ing.find_excisor(first_ms=0, n_ms=10, install=False)
        assert ing.get_excisor() is None
    finally:
        ing.close()
    plain.setflags(write=False)
    return plain, e, measured


def test_find_excisor_is_the_histogram_and_the_host_arithmetic_on_the_plain_output(eng, fm_plain):
    from gypsum_amd.excisor import excisor_from_hist
    plain, e, measured = fm_plain
    want, want_measured = excisor_from_hist(eng.spectrum_hist(plain[:10 * model.SCENE_N], model.SCENE_N), 16.0, 1)
    assert e == want and measured == want_measured


@pytest.mark.parametrize("block_ms", [1, 3, 10])
def test_a_handles_blocks_are_excised_then_levelled_as_the_stand_alone_calls_would(eng, scene_files, fm_plain, block_ms):
    """find_excisor(install) then calibrate: every block, from the start and after a seek, has the bits of gyp_excise_iq_dev followed
    by the stand-alone level on the handle's un-conditioned output; last_excised gives the stand-alone counts; host blocks are
    refused while the excisor is on; None gives back the original blocks."""
    n = model.SCENE_N
    plain, e_want, _ = fm_plain
    excised, counts, _ = eng.excise_iq(plain, n, e_want)
    assert counts.sum() > 0.05 * 256 * n_frames(n) * N_FILE_MS
    ing = IqFileIngest(scene_files["fm"], model.SCENE_FS, np.int8, block_ms=block_ms, depth=3, engine=eng)
    try:
        assert ing.total_ms == N_FILE_MS and ing.get_excisor() is None and ing.last_excised().size == 0
        e, _ = ing.find_excisor(first_ms=0, n_ms=10)
        assert e == e_want and ing.get_excisor() == e and ing.excisor == e
        level, _ = ing.calibrate(first_ms=0, n_ms=10)
        want = eng.condition_iq(excised, level)
        from gypsum_amd.level import default_target_rms, level_from_stats
        assert level == level_from_stats(eng.iq_stats(excised[:10 * n], n), n, default_target_rms(n))[0]   # measured on the excised output
        for at in (0, 5):
            ing.seek(at)
            per_block = []
            firsts, got = _drain(eng, ing, per_block)
            assert firsts == list(range(at, N_FILE_MS, block_ms)) and np.array_equal(_bits(got), _bits(want[at * n:])), (block_ms, at)
            for f, c in zip(firsts, per_block):
                assert c.tolist() == counts[f:f + block_ms].tolist(), f
        with pytest.raises(_lib.GypsumHipError, match="gyp_ingest_next_host") as err:
            ing.next_host_block()
        assert err.value.code == BAD
        with pytest.raises(_lib.GypsumHipError, match="gyp_ingest_set_excisor"):
            ing.set_excisor(Excisor(1.0, 9))
        assert ing.get_excisor() == e
        ing.set_excisor(None)
        ing.set_level(None)
        ing.seek(0)
        off = []
        assert np.array_equal(_bits(_drain(eng, ing, off)[1]), _bits(plain)) and ing.get_excisor() is None and not np.concatenate(off).any()
        ing.seek(0)
        assert ing.next_host_block() is not None
    finally:
        ing.close()


def test_the_chain_is_blanker_then_excisor_then_notches_then_level(eng, scene_files, fm_plain):
    """With all four installed a handle's output is each stage's stand-alone call applied in that order, bit for bit."""
    n, fs = model.SCENE_N, model.SCENE_FS
    plain, e, _ = fm_plain
    # (the jammer's envelope is constant: a blanker at the 95 % point of |x| takes the samples the noise lifts highest)
    b, tone, level = Blanker(0.0, 0.0, float(np.quantile(np.abs(plain), 0.95)), 1), 150_000, IqLevel(0.015625, -0.03125, 0.0625)
    ing = IqFileIngest(scene_files["fm"], fs, np.int8, block_ms=5, depth=3, engine=eng)
    try:
        ing.set_level(level)
        ing.set_notches([tone])
        ing.set_excisor(e)
        ing.set_blanker(b)
        assert (ing.blanker, ing.get_excisor(), ing.notches, ing.level) == (Blanker.from_record(b.record()), e, [tone], level)
        _, got = _drain(eng, ing)
        blanked, n_blanked = eng.blank_iq(plain, n, b)
        assert 0 < n_blanked.sum() < 0.5 * plain.size                         # the blanker does something, and not everything
        excised = eng.excise_iq(blanked, n, e)[0]
        want = eng.condition_iq(eng.notch_iq(excised, fs, n, [tone]), level)
        assert np.array_equal(_bits(got), _bits(want))
        other = eng.condition_iq(eng.notch_iq(eng.blank_iq(eng.excise_iq(plain, n, e)[0], n, b)[0], fs, n, [tone]), level)
        assert not np.array_equal(_bits(other), _bits(want))                   # the order is observable on this scene
        # find_excisor measures behind the blanker, without excisor, notches and level, and a refused call keeps everything
        found, _ = ing.find_excisor(first_ms=0, n_ms=10, install=False)
        from gypsum_amd.excisor import excisor_from_hist
        assert found == excisor_from_hist(eng.spectrum_hist(blanked[:10 * n], n), 16.0, 1)[0]
        for kw in (dict(first_ms=-1, n_ms=5), dict(first_ms=8, n_ms=5), dict(n_ms=0), dict(n_ms=1001), dict(threshold_over_median=0.0),
                   dict(threshold_over_median=np.inf), dict(guard=-1), dict(guard=9)):
            with pytest.raises(_lib.GypsumHipError, match="gyp_ingest_find_excisor") as err:
                ing.find_excisor(**kw)
            assert err.value.code == BAD
        assert (ing.blanker, ing.get_excisor(), ing.notches, ing.level) == (Blanker.from_record(b.record()), e, [tone], level)
        ing.seek(0)
        assert np.array_equal(_bits(_drain(eng, ing)[1]), _bits(want))
    finally:
        ing.close()


def test_find_excisor_does_not_depend_on_the_blocks_and_leaves_the_cursor(eng, scene_files, fm_plain):
    _, e_want, measured_want = fm_plain
    for block_ms in (1, 7):
        ing = IqFileIngest(scene_files["fm"], model.SCENE_FS, np.int8, block_ms=block_ms, depth=3, engine=eng)
        try:
            first = ing.next_device_block()[0]
            e, measured = ing.find_excisor(first_ms=0, n_ms=10, install=False)
            assert (e, measured) == (e_want, measured_want) and ing.get_excisor() is None
            assert first == 0 and ing.next_device_block()[0] == block_ms       # the cursor is where it was
        finally:
            ing.close()


def test_the_provider_finds_the_excisor_then_calibrates(eng, tmp_path):
    """An int8 recording at 2.048 Msps, noise under an FM jammer 40 dB above it, resampled to 2.046 Msps: the provider that measures
    equals a handle asked the same in the same order, and a provider given the excisor and the level it reports."""
    rng = np.random.default_rng(2048)
    count = 12 * 2048 + 1
    i = np.arange(count)
    x = rng.standard_normal(count) + 1j * rng.standard_normal(count) + 100.0 * np.exp(1j * (2.0 * np.pi * 0.106 * i + 20.0 * np.sin(2.0 * np.pi * 0.0015 * i)))
    path = tmp_path / "fm2048.i8"
    notch_model.scene_words(x.astype(np.complex64))[0].tofile(path)
    kw = dict(sample_component_data_type=np.int8, block_ms=5, engine=eng)
    prov = AntennaSampleProviderResampled(path, 2_048_000, find_excisor=True, calibrate=dict(first_ms=0, n_ms=8), **kw)
    ing = IqFileIngest(path, 2_046_000, np.int8, block_ms=5, depth=3, engine=eng, resample_from_hz=2_048_000)
    try:
        e, measured = ing.find_excisor()
        assert prov.excisor == e and prov.excised == measured and e.guard == 1
        level, _ = ing.calibrate(first_ms=0, n_ms=8)
        assert prov.level == level
        jammed = IqFileIngest(path, 2_046_000, np.int8, block_ms=5, depth=3, engine=eng, resample_from_hz=2_048_000)
        jammed_level, _ = jammed.calibrate(first_ms=0, n_ms=8)
        jammed.close()
        assert level.gain > 10.0 * jammed_level.gain                          # the jammer was 40 dB of the RMS
        got = prov.get_block(12).samples
        assert np.array_equal(_bits(got), _bits(_drain(eng, ing)[1]))
        fixed = AntennaSampleProviderResampled(path, 2_048_000, excise=e, level=level, **kw)
        assert np.array_equal(_bits(fixed.get_block(12).samples), _bits(got))
        fixed.close()
        with pytest.raises(ValueError, match="exclude"):
            AntennaSampleProviderResampled(path, 2_048_000, excise=e, find_excisor=True, **kw)
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


@pytest.mark.parametrize("kind", ["fm", "sweep"])
def test_a_jammed_recording_is_acquired_once_the_jammer_is_excised(eng, scene_files, kind):
    """The gated scenes (tests/test_excise_host.py) as int8 recordings at 2.046 Msps: through the ingest path gyp_acquire misses at
    least one planted satellite with no excisor and finds all four, at their code phases, after find_excisor and calibrate."""
    n, sats = model.SCENE_N, list(model.SCENE_SATS)
    ing = IqFileIngest(scene_files[kind], model.SCENE_FS, np.int8, block_ms=10, depth=3, engine=eng)

    def missed(results):
        return [sv for r, sv in zip(results, sats) if int(r["code_phase"]) != model.SCENE_SATS[sv][0] or float(r["strength"]) <= 3.0]

    try:
        f, n_ms, dev = ing.next_device_block()
        assert (f, n_ms) == (0, 10)
        raw = _acquire(eng, dev, 10, n, sats)
        print(kind, "raw:", [(int(r["doppler_hz"]), int(r["code_phase"]), round(float(r["strength"]), 2)) for r in raw])
        assert missed(raw)
        e, measured = ing.find_excisor(first_ms=0, n_ms=10)
        level, _ = ing.calibrate(first_ms=0, n_ms=10)
        ing.seek(0)
        f, n_ms, dev = ing.next_device_block()
        got = _acquire(eng, dev, 10, n, sats)
        share = ing.last_excised().sum() / (10.0 * n_frames(n) * 256)
        print(kind, "excisor", e, measured, "level", level, f"excised share {share:.4f}")
        print(kind, "excised:", [(int(r["doppler_hz"]), int(r["code_phase"]), round(float(r["strength"]), 2)) for r in got])
        assert not missed(got)
        assert 0.05 <= share <= 0.30
    finally:
        ing.close()


if __name__ == "__main__":
    # what MEASURED_X and MEASURED_Y are: model.excise32 against the float64 model on the inputs above
    worst_x = worst_y = 0.0
    for n, n_ms in SHAPES:
        for offset in (0, 1):
            flat, stride, rows = _case(n, n_ms, offset)
            for s in range(2):
                X, norm, has_nan = _reference(n, n_ms, offset, s)
                row = flat[rows[s]]
                w32 = model.window()
                for m in range(n_ms):
                    X32 = np.fft.fft(model.frames(row[m * n:(m + 1) * n]) * w32, axis=1)
                    assert X32.dtype == np.complex64
                    with np.errstate(invalid="ignore"):
                        worst_x = max(worst_x, float(np.nanmax(np.abs(X32 - X[m]) / norm[m][:, None])))
                for guard in GUARDS:
                    e = model.Excisor(THRESHOLD[s], guard)
                    y32, masks32, _ = model.excise32(row, n, e)
                    y64, _, _ = model.excise(row, n, e, masks=masks32)
                    touched = _touched(model.unpack_masks(masks32), n).reshape(-1)
                    with np.errstate(invalid="ignore"):
                        err = np.abs(y32.astype(np.complex128) - y64.astype(np.complex128)) / _sample_norm(norm, n).reshape(-1)
                    if touched.any():
                        worst_y = max(worst_y, float(np.nanmax(err[touched])))
        print(f"n {n}: spectrum {worst_x:.3g}, samples {worst_y:.3g} so far")
    print(f"MEASURED_X {worst_x:.3g}  MEASURED_Y {worst_y:.3g}")
