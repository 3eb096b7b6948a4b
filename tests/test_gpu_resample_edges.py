"""The on-device resampler at its edges: every word format x tap count at the rate edges against the float64 model with a
per-sample rounding bound, every tile shape (whole period, one sample short of it, the smallest and largest tile), batch and
window invariance, input indices past 2^31, degenerate windows, and the resampled ingest at other tap counts, at a trailing
partial sample, on a file shorter than a millisecond and on a sparse recording larger than 2^31 samples."""
from __future__ import annotations

import os

import numpy as np
import pytest

import resample_model as model
from gypsum_amd import _lib
from gypsum_amd import resample as rs
from gypsum_amd.engine import GypsumEngine
from gypsum_amd.ingest import IqFileIngest

pytestmark = pytest.mark.gpu

TAPS = [16, 24, 32, 48, 64]
FORMATS = {np.float32: _lib.GYP_FMT_F32, np.int8: _lib.GYP_FMT_I8, np.uint8: _lib.GYP_FMT_U8, np.int16: _lib.GYP_FMT_I16}
SCALES = {np.float32: 0.7, np.int8: 1.0 / 60, np.uint8: 1.0 / 60, np.int16: 1.0 / 8000}   # none of them a power of 2
# (fs_in, fs_out): L = N_out / gcd, M = N_in / gcd
EDGE_PAIRS = [(4_000_000, 4_092_000),     # g = 4, L = 1023, M = 1000
              (2_048_000, 2_046_000),     # g = 2, L = 1023, M = 1024
              (1_023_000, 2_046_000),     # exactly x2: L = 2, M = 1
              (1_025_000, 2_046_000),     # about x2, gcd 1: L = 2046, M = 1025
              (16_368_000, 8_184_000),    # exactly 0.5: L = 1, M = 2
              (16_367_000, 8_184_000),    # about 0.5, gcd 1: L = 8184, M = 16367 (chunked at every tile size)
              (50_000_000, 49_104_000)]   # L = 3069, M = 3125
DEFAULT_TILE = 4096


@pytest.fixture(scope="module")
def engines():
    """One engine per output rate, closed at the end of the module."""
    made = {}

    def get(fs_out: int) -> GypsumEngine:
        if fs_out not in made:
            eng = GypsumEngine(0)
            eng.set_stream_format(fs_out, fs_out // 1000)
            made[fs_out] = eng
        made[fs_out].debug_set("resample_tile_samples", DEFAULT_TILE)
        return made[fs_out]

    yield get
    for eng in made.values():
        eng.close()


def _words(rng, dtype, n_samples: int) -> np.ndarray:
    """Interleaved I,Q words of `dtype` spanning its range; one word in 20 is exactly zero."""
    w = rng.standard_normal(2 * n_samples)
    w[rng.random(2 * n_samples) < 0.05] = 0.0
    if dtype is np.float32:
        return w.astype(np.float32)
    if dtype is np.int16:
        return np.clip(np.rint(w * 8000), -32768, 32767).astype(np.int16)
    if dtype is np.int8:
        return np.clip(np.rint(w * 40), -128, 127).astype(np.int8)
    return np.clip(np.rint(w * 40) + 128, 0, 255).astype(np.uint8)


def _complex(words: np.ndarray, scale: float) -> np.ndarray:
    """x^ = word * float32(scale), exact in float64."""
    w = words.astype(np.float64) * np.float64(np.float32(scale))
    return w[0::2] + 1j * w[1::2]


def _run(eng, dtype, streams, in_stride, raw_first, raw_n, scale, fs_in, taps, first_ms, n_ms, out_stride=None, raw_ptr=None):
    """gyp_resample_iq_dev on `streams` (rows of words, laid out at in_stride samples); the outputs' slack is pre-filled with NaN
    so that a write outside [0, n_ms * N_out) of a stream shows."""
    n_out = eng.n
    out_stride = n_ms * n_out if out_stride is None else out_stride
    n_streams = len(streams)
    host = np.zeros((n_streams, 2 * in_stride), dtype=dtype)
    for s, w in enumerate(streams):
        host[s, :len(w)] = w
    d_raw = eng.alloc(max(1, host.nbytes)).upload(host) if raw_ptr is None else None
    nan = np.full(n_streams * out_stride, np.nan + 1j * np.nan, dtype=np.complex64)
    d_out = eng.alloc(nan.nbytes).upload(nan)
    eng.resample_iq_dev(FORMATS[dtype], d_raw.ptr.value if d_raw is not None else raw_ptr, n_streams, in_stride, raw_first, raw_n,
                        scale, fs_in, taps, first_ms, n_ms, out_stride, d_out.ptr.value)
    got = d_out.download(np.complex64, n_streams * out_stride).reshape(n_streams, out_stride)
    if d_raw is not None:
        d_raw.free()
    d_out.free()
    assert np.isnan(got[:, n_ms * n_out:].view(np.float32)).all()
    return got[:, :n_ms * n_out]


def _assert_within_rounding(got, x, fs_in, fs_out, first_ms, n_ms, taps, table, x_first=0, what=""):
    """Per output sample and component: |y_dev - y| <= (T + 2) 2^-24 sum_j |h_j| |x^_j|, y the model on the library's float32
    taps (T fma roundings plus the rounding of word * scale to float32).  An all-zero window gives exactly 0."""
    want = model.resample(x, fs_in, fs_out, first_ms, n_ms, taps, table, x_first)
    s_re, s_im = model.abs_sums(x, fs_in, fs_out, first_ms, n_ms, taps, table, x_first)
    eps = (taps + 2) * 2.0 ** -24
    g = got.astype(np.complex128)
    assert np.isfinite(g).all(), what
    for name, e, s in (("re", np.abs(g.real - want.real), s_re), ("im", np.abs(g.imag - want.imag), s_im)):
        bad = np.flatnonzero(e > eps * s)
        assert bad.size == 0, (what, name, bad[:5], e[bad[:5]], (eps * s)[bad[:5]])


@pytest.mark.parametrize("taps", TAPS)
@pytest.mark.parametrize("fs_in,fs_out", EDGE_PAIRS)
def test_values_within_the_rounding_bound(engines, fs_in, fs_out, taps):
    """All four word formats, three streams with ragged strides, output ms 1 .. 2 (the last ms's taps run past the end of the
    buffer): each sample within the fma chain's rounding bound of the model on the float32 design, and within 2e-6 max|x| of
    the model on the float64 design."""
    eng = engines(fs_out)
    rng = np.random.default_rng([fs_in, fs_out, taps])
    table = rs.design(fs_in, fs_out, taps)
    n_in, first_ms, n_ms = fs_in // 1000, 1, 2
    n_samples = (first_ms + n_ms) * n_in + 5
    in_stride, out_stride = n_samples + 37, n_ms * (fs_out // 1000) + 11
    for dtype in FORMATS:
        scale = SCALES[dtype]
        words = [_words(rng, dtype, n_samples) for _ in range(3)]
        got = _run(eng, dtype, words, in_stride, 0, n_samples, scale, fs_in, taps, first_ms, n_ms, out_stride)
        for s in range(3):
            x = _complex(words[s], scale)
            _assert_within_rounding(got[s], x, fs_in, fs_out, first_ms, n_ms, taps, table, what=(dtype.__name__, s))
        x = _complex(words[0], scale)
        want = model.resample(x, fs_in, fs_out, first_ms, n_ms, taps)
        assert np.abs(got[0].astype(np.complex128) - want).max() <= 2e-6 * np.abs(x).max(), dtype.__name__


def _tile_cases():
    for taps in TAPS:
        for fs_in, fs_out in ((1_025_000, 2_046_000), (2_048_000, 2_046_000)):
            M = fs_in // 1000
            yield fs_in, fs_out, taps, (M + taps - 1, M + taps - 2, 1024, 8192)
        yield 16_367_000, 8_184_000, taps, (1024, 8192)


@pytest.mark.parametrize("fs_in,fs_out,taps,tiles", list(_tile_cases()))
def test_every_tile_shape_gives_the_same_bits(engines, fs_in, fs_out, taps, tiles):
    """resample_tile_samples = M + T - 1 (one whole period, an exact LDS fit), M + T - 2 (the period cut into phase chunks), the
    smallest (1024) and the largest (8192, 64 KiB of LDS): the output equals the default tile's bit for bit.  9 ms make tiles
    of several periods run both the kernel's 4-period loop and its remainder loop."""
    eng = engines(fs_out)
    rng = np.random.default_rng([fs_in, taps])
    n_in, first_ms, n_ms = fs_in // 1000, 1, 9
    n_samples = (first_ms + n_ms) * n_in + 3
    words = [_words(rng, np.int16, n_samples) for _ in range(2)]
    args = (np.int16, words, n_samples + 5, 0, n_samples, 1.0 / 8000, fs_in, taps, first_ms, n_ms)
    want = _run(eng, *args)
    for tile in tiles:
        eng.debug_set("resample_tile_samples", tile)
        got = _run(eng, *args)
        eng.debug_set("resample_tile_samples", DEFAULT_TILE)
        assert got.tobytes() == want.tobytes(), tile
    x = _complex(words[1], 1.0 / 8000)
    _assert_within_rounding(want[1][:2 * (fs_out // 1000)], x, fs_in, fs_out, first_ms, 2, taps, rs.design(fs_in, fs_out, taps))


@pytest.mark.parametrize("taps", [16, 64])
@pytest.mark.parametrize("fs_in,fs_out", [(4_000_000, 4_092_000), (16_367_000, 8_184_000)])
def test_batch_and_window_invariance(engines, fs_in, fs_out, taps):
    """Stream s of a 37-stream call equals a 1-stream call on stream s's words; a call given only the samples its outputs need
    (raw_first_sample > 0, halo T/2 - 1 before and T/2 after) equals the whole-buffer call; bit for bit."""
    eng = engines(fs_out)
    rng = np.random.default_rng([fs_in, taps, 37])
    n_in, first_ms, n_ms = fs_in // 1000, 2, 2
    n_samples = (first_ms + n_ms + 1) * n_in
    scale = 1.0 / 60
    words = [_words(rng, np.int8, n_samples) for _ in range(37)]
    batch = _run(eng, np.int8, words, n_samples + 3, 0, n_samples, scale, fs_in, taps, first_ms, n_ms)
    w0, w1 = first_ms * n_in - (taps // 2 - 1), (first_ms + n_ms) * n_in + taps // 2
    for s in range(37):
        one = _run(eng, np.int8, [words[s]], n_samples, 0, n_samples, scale, fs_in, taps, first_ms, n_ms)
        assert one.tobytes() == batch[s].tobytes(), s
        if s % 9 == 0:
            win = words[s][2 * w0:2 * w1]
            got = _run(eng, np.int8, [win], w1 - w0 + 2, w0, w1 - w0, scale, fs_in, taps, first_ms, n_ms)
            assert got.tobytes() == batch[s].tobytes(), ("window", s)
    x = _complex(words[5], scale)
    _assert_within_rounding(batch[5], x, fs_in, fs_out, first_ms, n_ms, taps, rs.design(fs_in, fs_out, taps))


@pytest.mark.parametrize("taps", TAPS)
@pytest.mark.parametrize("fs_in,fs_out,far_ms", [(4_000_000, 4_092_000, 600_000), (16_367_000, 8_184_000, 140_000)])
def test_input_indices_past_2_31(engines, fs_in, fs_out, far_ms, taps):
    """The same window of words placed at output ms far_ms (input index about 2.4e9 > 2^31) and at ms 1: every output ms starts
    at m * N_in exactly, so the phases repeat and both calls give the same bits, and the far one matches the model there."""
    eng = engines(fs_out)
    n_in, n_ms = fs_in // 1000, 2
    assert far_ms * n_in > 2 ** 31
    rng = np.random.default_rng([far_ms, taps])
    span = n_ms * n_in + taps - 1
    words = _words(rng, np.int16, span)
    scale = 1.0 / 8000
    outs = []
    for m in (1, far_ms):
        first = m * n_in - (taps // 2 - 1)
        outs.append(_run(eng, np.int16, [words], span, first, span, scale, fs_in, taps, m, n_ms)[0])
    assert outs[0].tobytes() == outs[1].tobytes()
    assert np.abs(outs[1]).max() > 0
    first = far_ms * n_in - (taps // 2 - 1)
    _assert_within_rounding(outs[1], _complex(words, scale), fs_in, fs_out, far_ms, n_ms, taps, rs.design(fs_in, fs_out, taps),
                            x_first=first)


@pytest.mark.parametrize("taps", [16, 64])
def test_degenerate_windows_give_zeros(engines, taps):
    """raw_n_samples = 0 with a NULL buffer, and windows wholly after or wholly before every output's taps: all outputs are 0."""
    fs_in, fs_out = 4_000_000, 4_092_000
    eng = engines(fs_out)
    n_in, first_ms, n_ms = fs_in // 1000, 3, 2
    got = _run(eng, np.int16, [np.zeros(0, np.int16)] * 2, 4, 0, 0, 1.0, fs_in, taps, first_ms, n_ms, raw_ptr=0)
    assert not np.any(got.view(np.float32))
    words = np.full(2 * 500, 1000, dtype=np.int16)
    after = (first_ms + n_ms) * n_in + taps // 2                 # the first sample no output reads
    before = first_ms * n_in - (taps // 2 - 1) - 500            # ends at the last sample no output reads
    for raw_first in (after, after + 10 ** 9, before, -10 ** 9):
        got = _run(eng, np.int16, [words, words], 500, raw_first, 500, 1.0, fs_in, taps, first_ms, n_ms)
        assert not np.any(got.view(np.float32)), raw_first
    # one sample further in on either side does reach an output
    for raw_first in (after - 1, before + 1):
        got = _run(eng, np.int16, [words], 500, raw_first, 500, 1.0, fs_in, taps, first_ms, n_ms)
        assert np.count_nonzero(got) > 0, raw_first


# ---------------------------------------------------------------------------------------------- resampled ingest


def _read_all(eng, ing, start: int) -> np.ndarray:
    if start:
        ing.seek(start)
    got, expect_first = [], start
    while (blk := ing.next_device_block()) is not None:
        first, count, dev = blk
        assert first == expect_first
        expect_first += count
        buf = np.empty(count * ing.n, dtype=np.complex64)
        eng._check(eng.lib.gyp_memcpy_d2h(eng.ctx, _lib.ptr(buf), dev, buf.nbytes))
        got.append(buf)
    return np.concatenate(got) if got else np.zeros(0, np.complex64)


@pytest.mark.parametrize("dtype", list(FORMATS))
@pytest.mark.parametrize("taps", [16, 64])
@pytest.mark.parametrize("fs_in,fs_out", [(1_025_000, 2_046_000), (4_000_000, 4_092_000)])
def test_resampled_ingest_other_taps_and_formats(engines, tmp_path, fs_in, fs_out, taps, dtype):
    """gyp_ingest_open_resampled at T = 16 and 64 (its halo is T/2 - 1 before and T/2 after a block): block_ms 1 and 7, from ms 0
    and after a seek, equal the whole-recording call bit for bit; one extra word at the end (an I with no Q) reads as zero."""
    eng = engines(fs_out)
    n_in, n_out = fs_in // 1000, fs_out // 1000
    rng = np.random.default_rng([fs_in, taps, np.dtype(dtype).itemsize])
    words = _words(rng, dtype, 20 * n_in + 3)                 # ms 19's last taps lie past EOF
    scale = 1.0 if dtype is np.float32 else SCALES[dtype]     # set_scale is for integer recordings; float32 words go as they are
    total = 20
    whole = eng.resample(words, dtype, fs_in, 0, total, scale=scale, taps=taps)
    _assert_within_rounding(whole[-n_out:], _complex(words, scale), fs_in, fs_out, total - 1, 1, taps, rs.design(fs_in, fs_out, taps))
    extra = np.concatenate([words, np.array([100], dtype=dtype)])   # a trailing partial sample, within ms 19's halo
    for name, data in (("rec", words), ("partial", extra)):
        data.tofile(tmp_path / name)
        for block_ms in (1, 7):
            ing = IqFileIngest(tmp_path / name, fs_out, dtype, block_ms=block_ms, depth=3, engine=eng, resample_from_hz=fs_in,
                               taps=taps)
            if dtype is not np.float32:
                ing.set_scale(scale)
            assert (ing.total_ms, ing.n) == (total, n_out)
            assert _read_all(eng, ing, 0).tobytes() == whole.tobytes(), (name, block_ms)
            assert _read_all(eng, ing, 13).tobytes() == whole[13 * n_out:].tobytes(), (name, block_ms)
            ing.close()


def test_resampled_ingest_of_a_file_shorter_than_a_millisecond(engines, tmp_path):
    """(size - 1) // input ms bytes: 0 for a file of 0, 1 or exactly one input millisecond's bytes, and no device block; one
    byte more makes one millisecond."""
    fs_in, fs_out = 4_000_000, 4_092_000
    eng = engines(fs_out)
    ms_bytes = (fs_in // 1000) * 2 * 2
    for size, total in ((0, 0), (1, 0), (ms_bytes, 0), (ms_bytes + 1, 1)):
        path = tmp_path / f"short_{size}"
        path.write_bytes(np.ones(size // 2 + 1, dtype=np.int16).tobytes()[:size])
        ing = IqFileIngest(path, fs_out, np.int16, block_ms=4, depth=3, engine=eng, resample_from_hz=fs_in)
        assert ing.total_ms == total, size
        blocks = []
        while (blk := ing.next_device_block()) is not None:
            blocks.append(blk[:2])
        assert blocks == ([(0, 1)] if total else []), size
        ing.close()


def test_recording_larger_than_2_31_samples(engines, tmp_path):
    """A sparse int8 recording at 4.0 Msps of 2^31 + 5e5 samples (4.3 GB apparent) whose last 10 ms hold data: total_ms, a seek
    to the last ms, device blocks equal to those of a small file holding the same tail 2 ms in, and the plain (not resampled)
    ingest of the same file at 4.092 Msps equal to its words at the tail."""
    fs_in, fs_out = 4_000_000, 4_092_000
    n_in, n_out = fs_in // 1000, fs_out // 1000
    big_ms = 537_000                                           # 537000 * 4000 = 2.148e9 > 2^31 samples
    n_samples = big_ms * n_in + 5
    assert n_samples > 2 ** 31
    tail_first = (big_ms - 10) * n_in                          # sample index of the first word pair of data
    rng = np.random.default_rng(31)
    tail = _words(rng, np.int8, n_samples - tail_first)
    big = tmp_path / "big.bin"
    with open(big, "wb") as f:
        f.truncate(2 * n_samples)
    fd = os.open(big, os.O_WRONLY)
    try:
        assert os.pwrite(fd, tail.tobytes(), 2 * tail_first) == tail.nbytes
    finally:
        os.close(fd)
    st = os.stat(big)
    if st.st_blocks * 512 > 64 << 20:
        big.unlink()
        pytest.skip("the filesystem did not keep the recording sparse")
    small = tmp_path / "small.bin"
    lead_ms = 2
    np.concatenate([np.zeros(2 * lead_ms * n_in, np.int8), tail]).tofile(small)
    shift = big_ms - (lead_ms + 10)                            # big's ms k is small's ms k - shift
    assert (shift + lead_ms) * n_in == tail_first

    eng = engines(fs_out)
    scale = 1.0 / 60
    small_whole = eng.resample(np.fromfile(small, np.int8), np.int8, fs_in, 0, lead_ms + 10, scale=scale)
    for block_ms in (1, 3):
        ing_big = IqFileIngest(big, fs_out, np.int8, block_ms=block_ms, depth=3, engine=eng, resample_from_hz=fs_in)
        ing_small = IqFileIngest(small, fs_out, np.int8, block_ms=block_ms, depth=3, engine=eng, resample_from_hz=fs_in)
        ing_big.set_scale(scale)
        ing_small.set_scale(scale)
        assert (ing_big.total_ms, ing_small.total_ms) == (big_ms, lead_ms + 10)
        for back in (1, 4, 11):
            got = _read_all(eng, ing_big, big_ms - back)
            assert got.tobytes() == _read_all(eng, ing_small, lead_ms + 10 - back).tobytes(), (block_ms, back)
            assert got.tobytes() == small_whole[(lead_ms + 10 - back) * n_out:].tobytes(), (block_ms, back)
        assert np.abs(got).max() > 0
        ing_big.close()
        ing_small.close()

    # the plain ingest at the stream format's rate: complex64 of the words (scale 1), ms k at byte k * 4092 * 2
    n_plain = (2 * n_samples - 1) // (2 * n_out)
    ing = IqFileIngest(big, fs_out, np.int8, block_ms=2, depth=3, engine=eng)
    assert ing.total_ms == n_plain
    got = _read_all(eng, ing, n_plain - 5)
    s0 = (n_plain - 5) * n_out - tail_first
    assert s0 > 0
    w = tail[2 * s0:2 * (s0 + 5 * n_out)].astype(np.float32)
    assert got.tobytes() == (w[0::2] + 1j * w[1::2]).astype(np.complex64).tobytes()
    ing.close()
    big.unlink()
