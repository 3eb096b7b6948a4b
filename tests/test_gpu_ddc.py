"""The on-device down-converter (gyp_ddc_iq_dev, gyp_ingest_open_ddc): values against the float64 model of the contract with a
per-sample rounding bound, the mixer at input indices around 2^43, bit-identity across batches, windows, tile shapes, ingest
blocks, seeks and EOF, the gain and sign of the band, and real IF recordings run end to end."""
from __future__ import annotations

import numpy as np
import pytest

import ddc_model as model
from gypsum_amd import _lib, synth
from gypsum_amd import resample as rs
from gypsum_amd.engine import GypsumEngine
from gypsum_amd.ingest import IqFileIngest
from gypsum_amd.navigation_bit_intergrator import NavigationBitIntegratorBank

pytestmark = pytest.mark.gpu

FORMATS = {np.float32: _lib.GYP_FMT_F32, np.int8: _lib.GYP_FMT_I8, np.uint8: _lib.GYP_FMT_U8, np.int16: _lib.GYP_FMT_I16}
SCALES = {np.float32: 0.7, np.int8: 1.0 / 60, np.uint8: 1.0 / 60, np.int16: 1.0 / 8000}
DEFAULT_TILE = 4096


@pytest.fixture(scope="module")
def engines():
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


def _words(rng, dtype, n: int) -> np.ndarray:
    """Real words of `dtype` spanning its range; one word in 20 is exactly zero."""
    w = rng.standard_normal(n)
    w[rng.random(n) < 0.05] = 0.0
    if dtype is np.float32:
        return w.astype(np.float32)
    if dtype is np.int16:
        return np.clip(np.rint(w * 8000), -32768, 32767).astype(np.int16)
    if dtype is np.int8:
        return np.clip(np.rint(w * 40), -128, 127).astype(np.int8)
    return np.clip(np.rint(w * 40) + 128, 0, 255).astype(np.uint8)


def _real(words: np.ndarray, scale: float) -> np.ndarray:
    """x^ = word * float32(scale), exact in float64."""
    return words.astype(np.float64) * np.float64(np.float32(scale))


def _run(eng, dtype, streams, in_stride, raw_first, raw_n, scale, fs_in, if_hz, taps, first_ms, n_ms, out_stride=None):
    """gyp_ddc_iq_dev on `streams` (rows of real words at in_stride samples); the outputs' slack is pre-filled with NaN so that
    a write outside [0, n_ms * N_out) of a stream shows."""
    n_out = eng.n
    out_stride = n_ms * n_out if out_stride is None else out_stride
    host = np.zeros((len(streams), in_stride), dtype=dtype)
    for s, w in enumerate(streams):
        host[s, :len(w)] = w
    d_raw = eng.alloc(max(1, host.nbytes)).upload(host)
    nan = np.full(len(streams) * out_stride, np.nan + 1j * np.nan, dtype=np.complex64)
    d_out = eng.alloc(nan.nbytes).upload(nan)
    eng.ddc_iq_dev(FORMATS[dtype], d_raw.ptr.value, len(streams), in_stride, raw_first, raw_n, scale, fs_in, if_hz, taps, first_ms,
                   n_ms, out_stride, d_out.ptr.value)
    got = d_out.download(np.complex64, len(streams) * out_stride).reshape(len(streams), out_stride)
    d_raw.free()
    d_out.free()
    assert np.isnan(got[:, n_ms * n_out:].view(np.float32)).all()
    return got[:, :n_ms * n_out]


def _assert_within_rounding(got, x, fs_in, fs_out, if_hz, first_ms, n_ms, taps, x_first=0, what=""):
    """Per output sample and component: |y_dev - y| <= (T + 8) 2^-24 sum_j |h_j| |x^_j|, y the model on the library's float32
    taps.  With u = 2^-24 (half an ulp of 1), each term h_j z_j of the chain carries the rounding of word * scale (u |x|), the
    mixer's error (2^-22 = 4u per component of exp(-j theta)), the product x * mixer (u |x|), and the taps are the library's
    float32 ones: 6u |h_j| |x_j|.  T fma roundings add at most T u sum_j |h_j| |z_j| <= T u sum_j |h_j| |x_j|.  T + 6 to first
    order; T + 8 covers the second-order terms with room."""
    table = rs.ddc_design(fs_in, fs_out, if_hz, taps)
    want = model.ddc(x, fs_in, fs_out, if_hz, first_ms, n_ms, taps, table, x_first)
    s = model.abs_sums(x, fs_in, fs_out, first_ms, n_ms, taps, table, x_first)
    eps = (taps + 8) * 2.0 ** -24
    g = got.astype(np.complex128)
    assert np.isfinite(g).all(), what
    for name, e in (("re", np.abs(g.real - want.real)), ("im", np.abs(g.imag - want.imag))):
        bad = np.flatnonzero(e > eps * s)
        assert bad.size == 0, (what, name, bad[:5], e[bad[:5]], (eps * s)[bad[:5]])


# (fs_in, fs_out, if_hz): both signs, a non-kHz IF, a ratio with L > 1 and a chunked one (L = 1023, M = 2500)
VALUE_CASES = [(16_368_000, 4_092_000, 4_092_000), (16_368_000, 4_092_000, -4_092_000), (16_368_000, 4_092_000, 4_130_400),
               (38_192_000, 8_184_000, 9_548_000), (38_192_000, 8_184_000, -9_548_000), (5_000_000, 2_046_000, 1_250_000)]


@pytest.mark.parametrize("taps", model.TAPS)
@pytest.mark.parametrize("fs_in,fs_out,if_hz", VALUE_CASES)
def test_values_within_the_rounding_bound(engines, fs_in, fs_out, if_hz, taps):
    """All four word formats, three streams with ragged strides, output ms 1 .. 2 (the last ms's taps run past the end)."""
    eng = engines(fs_out)
    rng = np.random.default_rng([fs_in, fs_out, abs(if_hz), taps])
    n_in, first_ms, n_ms = fs_in // 1000, 1, 2
    n_samples = (first_ms + n_ms) * n_in + 5
    for dtype in FORMATS:
        scale = SCALES[dtype]
        words = [_words(rng, dtype, n_samples) for _ in range(3)]
        got = _run(eng, dtype, words, n_samples + 37, 0, n_samples, scale, fs_in, if_hz, taps, first_ms, n_ms,
                   n_ms * (fs_out // 1000) + 11)
        for s in range(3):
            _assert_within_rounding(got[s], _real(words[s], scale), fs_in, fs_out, if_hz, first_ms, n_ms, taps, what=(dtype.__name__, s))


def test_auto_taps_on_the_device(engines):
    """taps = 0 is the automatic T (96 at 38.192 -> 8.184), bit for bit."""
    eng = engines(8_184_000)
    rng = np.random.default_rng(96)
    words = _words(rng, np.int16, 3 * 38_192)
    args = (np.int16, [words], len(words), 0, len(words), 1.0 / 8000, 38_192_000, 9_548_000)
    assert _run(eng, *args, 0, 0, 3).tobytes() == _run(eng, *args, 96, 0, 3).tobytes()


@pytest.mark.parametrize("taps", [32, 128])
def test_mixer_values_within_2_22(engines, taps):
    """Isolated unit impulses (float32 words of 1.0, one per 2T samples): each output that sees one is h32 * m32 rounded once,
    so |y / h32 - exp(-j theta_i)| <= 2^-22 + 2^-24 per component.  Indices near 0 and near 2^43, IF 4_130_400 Hz."""
    fs_in, fs_out, if_hz = 16_368_000, 4_092_000, 4_130_400
    eng = engines(fs_out)
    table = rs.ddc_design(fs_in, fs_out, if_hz, taps).astype(np.float64)
    n_in, n_ms = fs_in // 1000, 4
    for m0 in (0, (1 << 43) // n_in):
        x_first = m0 * n_in
        n = n_ms * n_in
        x = np.zeros(n, dtype=np.float32)
        x[taps::2 * taps] = 1.0
        got = _run(eng, np.float32, [x], n, x_first, n, 1.0, fs_in, if_hz, taps, m0, n_ms)[0].astype(np.complex128)
        # every output: at most one impulse within its taps; h there from the float32 table, mixer exact
        want_h = model.ddc(x.astype(np.float64), fs_in, fs_out, if_hz, m0, n_ms, taps, table, x_first)
        hx = model.abs_sums(x.astype(np.float64), fs_in, fs_out, m0, n_ms, taps, table, x_first)
        ok = hx > 0
        assert ok.sum() > 1000
        bound = (2.0 ** -22 + 2.0 ** -24) * hx[ok]
        assert np.all(np.abs(got.real - want_h.real)[ok] <= bound)
        assert np.all(np.abs(got.imag - want_h.imag)[ok] <= bound)
        assert np.all(got[~ok] == 0)


def test_window_near_2_43_matches_the_model(engines):
    """A window whose absolute input index is about 2^43: (if_hz * i) overflows int64 there and a float phase accumulator would
    have drifted; the device matches the model's exact phase within the rounding bound, and the same words placed at index 0
    give other values (the mixer follows the absolute index)."""
    fs_in, fs_out, if_hz, taps = 16_368_000, 4_092_000, 4_130_400, 64
    eng = engines(fs_out)
    n_in, n_ms = fs_in // 1000, 2
    m0 = (1 << 43) // n_in
    assert if_hz * m0 * n_in > 2 ** 63
    rng = np.random.default_rng(43)
    span = n_ms * n_in + taps - 1
    words = _words(rng, np.int16, span)
    x_first = m0 * n_in - (taps // 2 - 1)
    got = _run(eng, np.int16, [words], span, x_first, span, 1.0 / 8000, fs_in, if_hz, taps, m0, n_ms)[0]
    _assert_within_rounding(got, _real(words, 1.0 / 8000), fs_in, fs_out, if_hz, m0, n_ms, taps, x_first, "2^43")
    near0 = _run(eng, np.int16, [words], span, n_in - (taps // 2 - 1), span, 1.0 / 8000, fs_in, if_hz, taps, 1, n_ms)[0]
    assert np.abs(near0 - got).max() > 1e-3 * np.abs(got).max()


@pytest.mark.parametrize("fs_in,fs_out,if_hz,taps", [(16_368_000, 4_092_000, 4_130_400, 64), (5_000_000, 2_046_000, -1_250_000, 48),
                                                     (38_192_000, 8_184_000, 9_548_000, 128)])
def test_batch_window_and_tile_invariance(engines, fs_in, fs_out, if_hz, taps):
    """Stream s of a 9-stream call equals a 1-stream call on it; a call given only the samples its outputs need (raw_first > 0)
    equals the whole-buffer call; resample_tile_samples 1024, 4096 and 8192 give the same bits; 9 ms run the kernel's 4-period
    loop and its remainder."""
    eng = engines(fs_out)
    rng = np.random.default_rng([fs_in, taps])
    n_in, first_ms, n_ms = fs_in // 1000, 2, 9
    n_samples = (first_ms + n_ms + 1) * n_in
    scale = 1.0 / 60
    words = [_words(rng, np.int8, n_samples) for _ in range(9)]
    batch = _run(eng, np.int8, words, n_samples + 3, 0, n_samples, scale, fs_in, if_hz, taps, first_ms, n_ms)
    for tile in (1024, 8192):
        eng.debug_set("resample_tile_samples", tile)
        got = _run(eng, np.int8, words, n_samples + 3, 0, n_samples, scale, fs_in, if_hz, taps, first_ms, n_ms)
        eng.debug_set("resample_tile_samples", DEFAULT_TILE)
        assert got.tobytes() == batch.tobytes(), tile
    w0, w1 = first_ms * n_in - (taps // 2 - 1), (first_ms + n_ms) * n_in + taps // 2
    for s in (0, 4, 8):
        one = _run(eng, np.int8, [words[s]], n_samples, 0, n_samples, scale, fs_in, if_hz, taps, first_ms, n_ms)
        assert one.tobytes() == batch[s].tobytes(), s
        win = words[s][w0:w1]
        got = _run(eng, np.int8, [win], w1 - w0 + 2, w0, w1 - w0, scale, fs_in, if_hz, taps, first_ms, n_ms)
        assert got.tobytes() == batch[s].tobytes(), ("window", s)
    _assert_within_rounding(batch[4][:2 * eng.n], _real(words[4], scale), fs_in, fs_out, if_hz, first_ms, 2, taps)


def test_refusals_on_the_device():
    eng = GypsumEngine(0)
    d = eng.alloc(1 << 16)
    with pytest.raises(_lib.GypsumHipError) as e:
        eng.ddc_iq_dev(_lib.GYP_FMT_I8, d.ptr.value, 1, 100, 0, 100, 1.0, 16_368_000, 4_092_000, 0, 0, 1, 4092, d.ptr.value)
    assert e.value.code == _lib.GYP_E_NO_FORMAT
    eng.set_stream_format(4_092_000, 4092)
    for fs_in, if_hz, taps, code in ((16_368_000, 0, 0, _lib.GYP_E_BAD_RATE), (16_368_000, 8_184_000, 0, _lib.GYP_E_BAD_RATE),
                                     (40_000_000, 10_000_000, 0, _lib.GYP_E_BAD_RATE), (16_368_500, 4_092_000, 0, _lib.GYP_E_BAD_RATE),
                                     (16_368_000, 4_092_000, 16, _lib.GYP_E_BAD_ARG), (16_368_000, 4_092_000, 100, _lib.GYP_E_BAD_ARG)):
        with pytest.raises(_lib.GypsumHipError) as e:
            eng.ddc_iq_dev(_lib.GYP_FMT_I8, d.ptr.value, 1, 100, 0, 100, 1.0, fs_in, if_hz, taps, 0, 1, 4092, d.ptr.value)
        assert e.value.code == code, (fs_in, if_hz, taps)
    d.free()
    eng.close()


def test_a_real_tone_comes_out_at_its_offset_with_half_amplitude(engines):
    """A cos(2 pi (if + d) t + phi) -> (A/2) exp(j (2 pi d t + phi)); read with the opposite IF sign, the same file gives the
    mirror image, (A/2) exp(-j (2 pi d t + phi)), not the tone at +d."""
    fs_in, fs_out, if_hz = 16_368_000, 4_092_000, 4_092_000
    eng = engines(fs_out)
    n_ms, A, d, phi = 4, 0.8, 312_345.0, 0.7
    t = np.arange(n_ms * 16_368) / fs_in
    x = (A * np.cos(2 * np.pi * (if_hz + d) * t + phi)).astype(np.float32)
    y = eng.ddc(x, np.float32, fs_in, if_hz)
    t_out = np.arange(len(y)) / fs_out
    want = 0.5 * A * np.exp(1j * (2 * np.pi * d * t_out + phi))
    assert np.abs(y - want)[64:-64].max() <= 2e-4 * A
    mirrored = eng.ddc(x, np.float32, fs_in, -if_hz)   # the band at -if holds the tone's other half, at -d
    assert np.abs(mirrored - np.conj(want))[64:-64].max() <= 2e-4 * A
    assert np.abs(mirrored - want)[64:-64].max() >= 0.5 * A


def test_ddc_ingest_is_bit_identical_to_the_whole_buffer_call(tmp_path, engines):
    """block_ms 1, 7 and 250, a seek, the last ms with its zero halo at EOF, and another tile size: every device block equals
    the whole-recording call bit for bit, and the mixer index is the absolute file index."""
    fs_in, fs_out, if_hz = 16_368_000, 4_092_000, 4_130_400
    rng = np.random.default_rng(7)
    n_in, n_out = fs_in // 1000, fs_out // 1000
    words = _words(rng, np.int16, 60 * n_in + 5)
    words.tofile(tmp_path / "rec")
    eng = engines(fs_out)
    scale = 1.0 / 8000
    total = (words.nbytes - 1) // (n_in * 2)
    assert total == 60
    whole = eng.ddc(words, np.int16, fs_in, if_hz, 0, total, scale=scale)
    for block_ms in (1, 7, 250):
        ing = IqFileIngest(tmp_path / "rec", fs_out, np.int16, block_ms=block_ms, depth=3, engine=eng, resample_from_hz=fs_in,
                           if_hz=if_hz)
        ing.set_scale(scale)
        assert (ing.total_ms, ing.n, ing.fs) == (total, n_out, fs_out)
        with pytest.raises(_lib.GypsumHipError):
            ing.next_host_block()
        for start in (0, 37):
            if start:
                ing.seek(start)
            got = []
            while (blk := ing.next_device_block()) is not None:
                first, count, dev = blk
                buf = np.empty(count * n_out, dtype=np.complex64)
                eng._check(eng.lib.gyp_memcpy_d2h(eng.ctx, _lib.ptr(buf), dev, buf.nbytes))
                got.append(buf)
            assert np.concatenate(got).tobytes() == whole[start * n_out:].tobytes(), (block_ms, start)
        t0, t1 = ing.times(0, total)
        assert t0[5] == round(5 * n_out / fs_out, 6) and t1[5] == round(6 * n_out / fs_out, 6)
        ing.close()
    eng.debug_set("resample_tile_samples", 1024)
    assert eng.ddc(words, np.int16, fs_in, if_hz, 0, total, scale=scale).tobytes() == whole.tobytes()
    eng.debug_set("resample_tile_samples", DEFAULT_TILE)
    _assert_within_rounding(whole[-n_out:], _real(words, scale), fs_in, fs_out, if_hz, total - 1, 1, 64, what="EOF")


def _recording(tmp_path, fs_in, fs_out, if_hz, dtype, n_ms, seed):
    scene = synth.random_scene(fs_out, n_ms, 3, seed, max_code_phase=2046, noise_sigma=0.02)
    x = synth.render_real_if(scene, fs_in, if_hz)
    if dtype is np.int16:
        words, scale = np.clip(np.rint(x * 1000), -32768, 32767).astype(np.int16), 1e-3
    else:                                                    # an 8-bit front end, noise sigma about 6 LSB
        words, scale = np.clip(np.rint(x * 200), -128, 127).astype(np.int8), 5e-3
    path = tmp_path / f"rec_{fs_in}.bin"
    words.tofile(path)
    return scene, words, scale, path


@pytest.mark.parametrize("fs_in,fs_out,if_hz,dtype,seed", [(16_368_000, 4_092_000, 4_092_000, np.int8, 43),
                                                           (38_192_000, 8_184_000, -9_548_000, np.int16, 41)])
def test_real_if_recording_to_navigation_bits(tmp_path, fs_in, fs_out, if_hz, dtype, seed):
    """Modelled on test_recording_at_a_round_rate_to_navigation_bits: acquisition on the first 10 down-converted ms finds every
    planted satellite at code phase round(tau * fs_out) +- 1 and its Doppler +- 50 Hz; tracking the ingest's device blocks gives
    the records of track_block on the whole down-converted recording bit for bit, and decodes the bits up to polarity."""
    n_ms = 2600
    n = fs_out // 1000
    scene, words, scale, path = _recording(tmp_path, fs_in, fs_out, if_hz, dtype, n_ms, seed)
    eng = GypsumEngine(0)
    eng.set_stream_format(fs_out, n)
    ing = IqFileIngest(path, fs_out, dtype, block_ms=250, depth=3, engine=eng, resample_from_hz=fs_in, if_hz=if_hz)
    ing.set_scale(scale)
    total = ing.total_ms
    whole = eng.ddc(words, dtype, fs_in, if_hz, 0, total, scale=scale)
    sat_ids = [s.sat_id for s in scene.sats]
    acq = eng.acquire(whole[:10 * n], 1, 10, sat_ids)
    for s, a in zip(scene.sats, acq):
        assert a["sat_id"] == s.sat_id and a["strength"] > 3
        assert abs(int(a["code_phase"]) - round(s.code_phase / scene.fs * fs_out)) <= 1, (s, a)
        assert abs(float(a["doppler_hz"]) - s.doppler_hz) <= 50, (s, a)
    inits = np.zeros(len(sat_ids), dtype=_lib.CHAN_INIT)
    for i, a in enumerate(acq):
        inits[i] = (0, a["sat_id"], a["doppler_hz"], a["carrier_phase"], a["code_phase"], 0)
    start_all, _ = ing.times(0, total)
    want = eng.create_bank(inits).track_block(whole[9 * n:], 1, total - 9, start_all[9:])

    bank = eng.create_bank(inits)
    bits = NavigationBitIntegratorBank(len(sat_ids))
    ing.seek(9)
    d_times = eng.alloc(250 * 8)
    d_rec = eng.alloc(len(sat_ids) * 250 * _lib.TRACK_REC.itemsize)
    recs, events = [], []
    while (blk := ing.next_device_block()) is not None:
        first, count, dev = blk
        t0, t1 = ing.times(first, count)
        d_times.upload(t0)
        bank.track_block_dev(dev, 0, count, d_times.ptr.value, d_rec.ptr.value)
        r = d_rec.download(_lib.TRACK_REC, len(sat_ids) * count).reshape(len(sat_ids), count)
        recs.append(r)
        events.append(bits.push_block(r, t0, t1))
    got = np.concatenate(recs, axis=1)
    events = np.concatenate(events)
    assert got.tobytes() == want.tobytes()
    for c, sat in enumerate(scene.sats):
        mine = events[events["channel"] == c]
        known = mine[mine["bit_value"] != _lib.GYP_BIT_UNKNOWN]
        assert len(known) > 30, (sat.sat_id, len(mine))
        known = known[-25:]
        ms_of_bit = np.rint(known["receiver_timestamp"] * 1000).astype(int)
        sent = np.array([synth.nav_symbol_at(sat, int(m) + 10) for m in ms_of_bit])
        agree = np.mean(known["bit_value"] * 2 - 1 == sent)
        assert max(agree, 1 - agree) == 1.0, (sat.sat_id, agree)
    ing.close()
    eng.close()


def test_batched_receiver_on_a_real_if_recording(tmp_path):
    from gypsum_amd.antenna_sample_provider import AntennaSampleProviderResampled
    from gypsum_amd.gps_ca_prn_codes import GpsSatelliteId
    from gypsum_amd.radio_input import InputFileInfo
    from gypsum_amd.receiver import BatchedGpsReceiver

    fs_in, if_hz = 16_368_000, 4_092_000
    scene, words, scale, path = _recording(tmp_path, fs_in, 8_184_000, if_hz, np.int8, 900, 47)
    prov = AntennaSampleProviderResampled(InputFileInfo.real_if(path, fs_in, if_hz, np.int8), scale=scale)
    attrs = prov.get_attributes()
    assert (attrs.samples_per_second, attrs.samples_per_prn_transmission) == (8_184_000, 8184)   # default_ddc_rate
    planted = {s.sat_id for s in scene.sats}
    brx = BatchedGpsReceiver(prov, only_acquire_satellite_ids=[GpsSatelliteId(i) for i in sorted(planted | {1, 2})])
    brx.run(2000)
    assert brx.steps_done == prov.total_ms == 899
    assert {s.id for s in brx.tracked_satellite_ids_to_tracking_params} == planted
    prov.close()
