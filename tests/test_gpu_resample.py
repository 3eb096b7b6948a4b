"""The on-device resampler (gyp_resample_iq_dev, gyp_ingest_open_resampled): values against the float64 model of the
contract, bit-identical blocks / windows / seeks, and recordings at 4.000 and 2.048 Msps run end to end."""
from __future__ import annotations

import numpy as np
import pytest

import resample_model as model
from gypsum_amd import _lib, synth
from gypsum_amd.engine import GypsumEngine
from gypsum_amd.ingest import IqFileIngest
from gypsum_amd.navigation_bit_intergrator import NavigationBitIntegratorBank

pytestmark = pytest.mark.gpu

PAIRS = [(2_048_000, 2_046_000), (4_000_000, 4_092_000), (5_000_000, 5_115_000), (10_000_000, 8_184_000),
         (20_000_000, 20_460_000), (25_000_000, 20_460_000), (16_368_000, 8_184_000), (50_000_000, 49_104_000)]
FORMATS = {np.float32: _lib.GYP_FMT_F32, np.int8: _lib.GYP_FMT_I8, np.uint8: _lib.GYP_FMT_U8, np.int16: _lib.GYP_FMT_I16}


def _engine(fs_out: int) -> GypsumEngine:
    eng = GypsumEngine(0)
    eng.set_stream_format(fs_out, fs_out // 1000)
    return eng


def _words(rng, dtype, n_samples: int, fs: int) -> np.ndarray:
    """Noise plus two tones, as interleaved words of `dtype`."""
    t = np.arange(n_samples) / fs
    x = 0.3 * (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples))
    x += 0.5 * np.exp(2j * np.pi * 0.11 * fs * t) + 0.25 * np.exp(-2j * np.pi * 0.3 * fs * t + 1.0)
    w = np.empty(2 * n_samples)
    w[0::2], w[1::2] = x.real, x.imag
    if dtype is np.float32:
        return w.astype(np.float32)
    if dtype is np.int16:
        return np.clip(np.rint(w * 8000), -32768, 32767).astype(np.int16)
    if dtype is np.int8:
        return np.clip(np.rint(w * 60), -128, 127).astype(np.int8)
    return np.clip(np.rint(w * 60) + 128, 0, 255).astype(np.uint8)


def _complex(words: np.ndarray, scale: float) -> np.ndarray:
    w = words.astype(np.float64) * np.float64(np.float32(scale))
    return w[0::2] + 1j * w[1::2]


@pytest.mark.parametrize("fs_in,fs_out", PAIRS)
def test_values_match_the_float64_model(fs_in, fs_out):
    """Two streams with ragged strides, all four word formats: within 2e-6 max|x| of the float64 model; a windowed call
    (raw_first_sample != 0, only the samples the outputs need) is bit-identical to the whole-buffer call."""
    rng = np.random.default_rng(fs_in ^ fs_out)
    eng = _engine(fs_out)
    n_in, n_out, n_ms, first_ms = fs_in // 1000, fs_out // 1000, 3, 1
    n_samples = (n_ms + first_ms) * n_in + 5                  # the last millisecond's taps run past the end: zeros
    in_stride, out_stride = n_samples + 37, n_ms * n_out + 11
    for dtype, fmt in FORMATS.items():
        scale = 1.0 if dtype is np.float32 else 1.0 / 64
        words = [_words(rng, dtype, n_samples, fs_in) for _ in range(2)]
        host = np.zeros((2, 2 * in_stride), dtype=dtype)
        for s in range(2):
            host[s, :2 * n_samples] = words[s]
        d_raw = eng.alloc(host.nbytes).upload(host)
        d_out = eng.alloc(2 * out_stride * 8)
        eng.resample_iq_dev(fmt, d_raw.ptr.value, 2, in_stride, 0, n_samples, scale, fs_in, 32, first_ms, n_ms, out_stride, d_out.ptr.value)
        got = d_out.download(np.complex64, 2 * out_stride).reshape(2, out_stride)[:, :n_ms * n_out]
        for s in range(2):
            x = _complex(words[s], scale)
            want = model.resample(x, fs_in, fs_out, first_ms, n_ms)
            err = np.abs(got[s].astype(np.complex128) - want).max()
            assert err <= 2e-6 * np.abs(x).max(), (dtype.__name__, s, err)
        # windowed: stream 1's samples [w0, w1) only, w0 > 0
        w0 = first_ms * n_in - 15
        w1 = min(n_samples, (first_ms + n_ms) * n_in + 16)
        win = np.ascontiguousarray(words[1][2 * w0:2 * w1])
        d_win = eng.alloc(win.nbytes).upload(win)
        d_o2 = eng.alloc(n_ms * n_out * 8)
        eng.resample_iq_dev(fmt, d_win.ptr.value, 1, w1 - w0, w0, w1 - w0, scale, fs_in, 32, first_ms, n_ms, n_ms * n_out, d_o2.ptr.value)
        assert d_o2.download(np.complex64, n_ms * n_out).tobytes() == got[1].tobytes(), dtype.__name__
        for b in (d_raw, d_out, d_win, d_o2):
            b.free()
    eng.close()


def test_refusals_on_the_device():
    eng = GypsumEngine(0)
    d = eng.alloc(1 << 16)
    with pytest.raises(_lib.GypsumHipError) as e:         # no stream format yet
        eng.resample_iq_dev(_lib.GYP_FMT_I16, d.ptr.value, 1, 100, 0, 100, 1.0, 4_000_000, 32, 0, 1, 4092, d.ptr.value)
    assert e.value.code == _lib.GYP_E_NO_FORMAT
    eng.set_stream_format(4_092_000, 4092)
    for fs_in, taps, code in ((4_092_000, 32, _lib.GYP_E_BAD_RATE), (1_000_000, 32, _lib.GYP_E_BAD_RATE),
                              (4_000_500, 32, _lib.GYP_E_BAD_RATE), (4_000_000, 20, _lib.GYP_E_BAD_ARG)):
        with pytest.raises(_lib.GypsumHipError) as e:
            eng.resample_iq_dev(_lib.GYP_FMT_I16, d.ptr.value, 1, 100, 0, 100, 1.0, fs_in, taps, 0, 1, 4092, d.ptr.value)
        assert e.value.code == code, (fs_in, taps)
    d.free()
    eng.close()


def test_resampled_ingest_is_bit_identical_to_the_whole_buffer_call(tmp_path):
    """block_ms 1, 7 and 250, a seek, the last millisecond with its zero halo at EOF, and a different tile size: every
    device block equals the whole-recording call bit for bit."""
    fs_in, fs_out = 4_000_000, 4_092_000
    rng = np.random.default_rng(7)
    n_in, n_out = fs_in // 1000, fs_out // 1000
    words = _words(rng, np.int16, 120 * n_in + 5, fs_in)   # ms 119's last taps lie past EOF
    words.tofile(tmp_path / "rec")
    eng = _engine(fs_out)
    scale = 1.0 / 8000
    total = (words.nbytes - 1) // (n_in * 4)
    assert total == 120
    whole = eng.resample(words, np.int16, fs_in, 0, total, scale=scale)
    for block_ms in (1, 7, 250):
        ing = IqFileIngest(tmp_path / "rec", fs_out, np.int16, block_ms=block_ms, depth=3, engine=eng, resample_from_hz=fs_in)
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
                assert first == start + sum(len(g) for g in got) // n_out
                buf = np.empty(count * n_out, dtype=np.complex64)
                eng._check(eng.lib.gyp_memcpy_d2h(eng.ctx, _lib.ptr(buf), dev, buf.nbytes))
                got.append(buf)
            got = np.concatenate(got)
            assert got.tobytes() == whole[start * n_out:].tobytes(), (block_ms, start)
        t0, t1 = ing.times(0, total)
        assert t0[5] == round(5 * n_out / fs_out, 6) and t1[5] == round(6 * n_out / fs_out, 6)
        ing.close()
    eng.debug_set("resample_tile_samples", 1024)          # another launch shape: same samples
    assert eng.resample(words, np.int16, fs_in, 0, total, scale=scale).tobytes() == whole.tobytes()
    # the last millisecond reads past the end of the file: zeros, as in a buffer that ends there
    x = _complex(words, scale)
    np.testing.assert_allclose(whole[-n_out:], model.resample(x, fs_in, fs_out, total - 1, 1), atol=2e-6 * np.abs(x).max(), rtol=0)
    eng.close()


def _recording(tmp_path, fs_in, fs_out, dtype, n_ms, seed, lock_regime=True):
    # lock_regime: a*N ~ U(14, 27) and a noise level at which most channels lock; otherwise test_file_to_navigation_bits's
    # regime (a*N = 20.46, sigma 0.02 at 2.046 Msps), where every channel decodes
    scene = (synth.lock_regime_scene(fs_out, n_ms, seed) if lock_regime else
             synth.random_scene(fs_out, n_ms, 3, seed, max_code_phase=2046, noise_sigma=0.02))
    iq = synth.render_at_rate(scene, fs_in)
    w = np.empty(2 * len(iq))
    w[0::2], w[1::2] = iq.real, iq.imag
    if dtype is np.int16:
        words, scale = np.clip(np.rint(w * 1000), -32768, 32767).astype(np.int16), 1e-3
    else:                                                    # an 8-bit front end (HackRF style), noise sigma about 3 LSB
        words, scale = np.clip(np.rint(w * 200), -128, 127).astype(np.int8), 5e-3
    path = tmp_path / f"rec_{fs_in}.bin"
    words.tofile(path)
    return scene, words, scale, path


# 8-bit input at 2.048 Msps is int8 here: an RTL-SDR's uint8 words carry their 127.5 offset through the ingest and the
# resampler (word * scale, as np.fromfile gives them), and a DC term 75 times the satellites' amplitude swamps acquisition.
@pytest.mark.parametrize("fs_in,fs_out,dtype,seed,lock_regime", [(4_000_000, 4_092_000, np.int16, 41, True),
                                                                 (2_048_000, 2_046_000, np.int8, 43, False)])
def test_recording_at_a_round_rate_to_navigation_bits(tmp_path, fs_in, fs_out, dtype, seed, lock_regime):
    """Modelled on test_file_to_navigation_bits: acquisition on the first 10 resampled ms finds every planted satellite at
    code phase round(tau * fs_out) +- 1 and its Doppler +- 50 Hz; tracking the ingest's device blocks gives the records of
    track_block on the whole resampled recording, bit for bit, and decodes the transmitted bits up to polarity."""
    n_ms = 2600
    n = fs_out // 1000
    scene, words, scale, path = _recording(tmp_path, fs_in, fs_out, dtype, n_ms, seed, lock_regime)
    eng = _engine(fs_out)
    ing = IqFileIngest(path, fs_out, dtype, block_ms=250, depth=3, engine=eng, resample_from_hz=fs_in)
    ing.set_scale(scale)
    total = ing.total_ms
    whole = eng.resample(words, dtype, fs_in, 0, total, scale=scale)
    sat_ids = [s.sat_id for s in scene.sats]
    acq = eng.acquire(whole[:10 * n], 1, 10, sat_ids)
    for s, a in zip(scene.sats, acq):
        assert a["sat_id"] == s.sat_id and a["strength"] > 3
        assert abs(int(a["code_phase"]) - round(s.code_phase / scene.fs * fs_out)) <= 1, (s, a)
        assert abs(float(a["doppler_hz"]) - s.doppler_hz) <= 50, (s, a)
    inits = np.zeros(len(sat_ids), dtype=_lib.CHAN_INIT)
    for i, a in enumerate(acq):
        inits[i] = (0, a["sat_id"], a["doppler_hz"], a["carrier_phase"], a["code_phase"], 0)
    start_all, end_all = ing.times(0, total)
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
        known = known[-25:]                                  # once the loops have pulled in
        ms_of_bit = np.rint(known["receiver_timestamp"] * 1000).astype(int)
        sent = np.array([synth.nav_symbol_at(sat, int(m) + 10) for m in ms_of_bit])
        agree = np.mean(known["bit_value"] * 2 - 1 == sent)
        assert max(agree, 1 - agree) == 1.0, (sat.sat_id, agree)
    ing.close()
    eng.close()


def test_batched_receiver_on_a_4_msps_recording(tmp_path):
    from gypsum_amd.antenna_sample_provider import AntennaSampleProviderResampled
    from gypsum_amd.radio_input import InputFileInfo
    from gypsum_amd.receiver import BatchedGpsReceiver
    from gypsum_amd.gps_ca_prn_codes import GpsSatelliteId

    scene, words, scale, path = _recording(tmp_path, 4_000_000, 4_092_000, np.int16, 900, 41)
    prov = AntennaSampleProviderResampled(InputFileInfo.raw(path, 4_000_000, np.int16), scale=scale)
    attrs = prov.get_attributes()
    assert (attrs.samples_per_second, attrs.samples_per_prn_transmission) == (4_092_000, 4092)
    planted = {s.sat_id for s in scene.sats}
    brx = BatchedGpsReceiver(prov, only_acquire_satellite_ids=[GpsSatelliteId(i) for i in sorted(planted | {1, 2})])
    events = brx.run(2000)
    assert brx.steps_done == prov.total_ms == 899
    assert {s.id for s in brx.tracked_satellite_ids_to_tracking_params} == planted
    for sid in planted:
        assert len(events.get(GpsSatelliteId(sid), [])) > 15, sid
    prov.close()
