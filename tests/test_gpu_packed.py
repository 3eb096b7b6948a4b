"""Packed recordings on the device (gyp_unpack_iq_dev, gyp_resample_packed_dev, gyp_ingest_open_packed).  The oracle is the int8
path on the twin file whose words are the levels: preset levels are exact in int8, so every packed result must equal it bit for
bit -- native-rate unpacking, resampling and down-conversion, in blocks of 1, 7 and 250 ms, after seeks to odd milliseconds, up
to EOF on files ending in a partial sample, with scale != 1; the device entries on several streams at every bit offset; and
recordings run through AntennaSampleProviderResampled and BatchedGpsReceiver."""
from __future__ import annotations

import numpy as np
import pytest

from gypsum_amd import _lib, synth
from gypsum_amd import packing as pk
from gypsum_amd.engine import GypsumEngine
from gypsum_amd.ingest import IqFileIngest

pytestmark = pytest.mark.gpu

PRESETS = {"sm": pk.sign_magnitude, "tc": pk.twos_complement, "ob": pk.offset_binary}


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(fs_out: int) -> GypsumEngine:
        if fs_out not in made:
            eng = GypsumEngine(0)
            eng.set_stream_format(fs_out, fs_out // 1000)
            made[fs_out] = eng
        return made[fs_out]

    yield get
    for eng in made.values():
        eng.close()


def _files(tmp_path, p: pk.Packing, n_samples: int, seed: int, tail_words: int = 0):
    """Random codes for n_samples samples (+ tail words of a partial sample) as a packed file and its int8 twin."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 1 << p.bits, n_samples * p.words_per_sample + tail_words)
    packed, twin = tmp_path / f"p{seed}.bin", tmp_path / f"t{seed}.bin"
    packed.write_bytes(pk.pack(codes, p))
    n = p.file_samples(packed.stat().st_size)
    whole = np.zeros(n * p.words_per_sample, dtype=np.int64)
    k = min(whole.size, codes.size)
    whole[:k] = codes[:k]
    np.asarray(p.levels).astype(np.int8)[whole].tofile(twin)
    return packed, twin, n


def _drain(eng, ing, first=None):
    """Every device block from the handle's position on, downloaded: (first ms, concatenated samples)."""
    got, start = [], None
    while (blk := ing.next_device_block()) is not None:
        f, count, dev = blk
        start = f if start is None else start
        buf = np.empty(count * ing.n, dtype=np.complex64)
        eng._check(eng.lib.gyp_memcpy_d2h(eng.ctx, _lib.ptr(buf), _lib.C.c_void_p(dev), buf.nbytes))
        got.append(buf)
    return start, (np.concatenate(got) if got else np.empty(0, np.complex64))


def _same(a, b) -> bool:
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _compare_ingests(eng, packed, twin, p, fs_out, fs_in, if_hz, block_ms, scale, seeks=(), taps=None):
    """The packed handle and the int8 twin's handle give the same total_ms, times and device blocks, from the start and after
    each seek."""
    kw = dict(engine=eng, block_ms=block_ms, depth=3)
    if fs_in == fs_out and not p.real:
        a = IqFileIngest(packed, fs_out, packing=p, **kw)
        b = IqFileIngest(twin, fs_out, np.int8, **kw)
    else:
        a = IqFileIngest(packed, fs_out, packing=p, resample_from_hz=fs_in, if_hz=if_hz, taps=taps, **kw)
        b = IqFileIngest(twin, fs_out, np.int8, resample_from_hz=fs_in, if_hz=if_hz, taps=taps, **kw)
    try:
        if scale != 1.0:
            a.set_scale(scale)
            b.set_scale(scale)
        assert a.total_ms == b.total_ms > 0
        ta, tb = a.times(0, a.total_ms), b.times(0, b.total_ms)
        assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])
        for at in (None, *seeks):
            if at is not None:
                a.seek(at)
                b.seek(at)
            fa, xa = _drain(eng, a)
            fb, xb = _drain(eng, b)
            assert fa == fb and xa.size == (a.total_ms - (at or 0)) * eng.n
            assert _same(xa, xb), (block_ms, at)
            assert np.isfinite(xa.view(np.float32)).all()
        return a.total_ms
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("bits", [1, 2, 4])
@pytest.mark.parametrize("order", ["msb", "lsb"])
@pytest.mark.parametrize("preset", ["sm", "tc", "ob"])
def test_native_rate_iq_equals_the_int8_twin(tmp_path, engines, k, bits, order, preset):
    fs = 1_023_000 * k
    eng = engines(fs)
    p = PRESETS[preset](bits, order=order)
    n_ms = 23
    i = (k + bits + len(order) + len(preset)) % 3
    block_ms = (1, 7, 250)[i]
    packed, twin, n = _files(tmp_path, p, n_ms * fs // 1000 + 517, seed=k * 100 + bits * 10 + len(order), tail_words=1)
    total = _compare_ingests(eng, packed, twin, p, fs, fs, None, block_ms, (1.0, 1.0 / 7, 0.03)[i], seeks=(5, 11, 1))
    assert total == (n - 1) // (fs // 1000)


@pytest.mark.parametrize("fs_in,fs_out", [(2_048_000, 2_046_000), (4_000_000, 4_092_000)])
@pytest.mark.parametrize("bits", [1, 2, 4])
@pytest.mark.parametrize("order", ["msb", "lsb"])
def test_resampled_iq_equals_the_int8_twin(tmp_path, engines, fs_in, fs_out, bits, order):
    eng = engines(fs_out)
    p = pk.sign_magnitude(bits, order=order)          # code 0 is +1: padding by code 0 would show
    # files end 5, 333 and 2 samples past a millisecond edge: the last blocks' halos reach past EOF except in the middle case
    for j, block_ms in enumerate((1, 7, 250)):
        packed, twin, _ = _files(tmp_path, p, 19 * fs_in // 1000 + (5, 333, 2)[j], seed=bits * 10 + j + len(order), tail_words=j % 2)
        _compare_ingests(eng, packed, twin, p, fs_out, fs_in, None, block_ms, (1.0, 0.25, 1.0 / 3)[j], seeks=(3, 13, 0),
                         taps=(16, 32, 64)[j])


@pytest.mark.parametrize("fs_in,if_hz,fs_out", [(16_368_000, 4_092_000, 4_092_000), (38_192_000, 9_548_000, 8_184_000)])
@pytest.mark.parametrize("bits", [1, 2, 4])
@pytest.mark.parametrize("order", ["msb", "lsb"])
def test_ddc_real_equals_the_int8_twin(tmp_path, engines, fs_in, if_hz, fs_out, bits, order):
    eng = engines(fs_out)
    p = pk.sign_magnitude(bits, real=True, order=order)
    for j, block_ms in enumerate((1, 7, 250)):
        # 1-bit: the byte holds 8 samples, so a partial last byte is whole samples; 2 / 4 bits end on a sample edge or mid-byte
        packed, twin, _ = _files(tmp_path, p, 11 * fs_in // 1000 + 1001 * j + 3, seed=bits * 10 + j + len(order))
        _compare_ingests(eng, packed, twin, p, fs_out, fs_in, if_hz, block_ms, (1.0 / 5, 1.0, 0.125)[j], seeks=(7, 1))


def _bit0s(p):
    return list(range(0, 8, p.sample_bits))


def _streams(rng, p, n_streams, n_samples, bit0, stride_bytes):
    """n_streams rows of stride_bytes bytes, stream s's samples from bit bit0 of its first byte; every other bit random (never
    zero-filled), and the int8 twin rows of the same samples."""
    codes = rng.integers(0, 1 << p.bits, (n_streams, n_samples * p.words_per_sample))
    raw = rng.integers(0, 256, (n_streams, stride_bytes)).astype(np.uint8)
    lead = bit0 // p.bits
    for s in range(n_streams):
        filler = rng.integers(0, 1 << p.bits, lead)
        body = np.frombuffer(pk.pack(np.concatenate([filler, codes[s]]), p), dtype=np.uint8)
        # keep the random bits after the last sample: rebuild the last byte from both
        used_bits = bit0 + n_samples * p.sample_bits
        full = used_bits // 8
        raw[s, :full] = body[:full]
        if used_bits % 8:
            keep = (1 << (8 - used_bits % 8)) - 1 if p.order == "msb" else ~((1 << (used_bits % 8)) - 1) & 0xFF
            raw[s, full] = (int(raw[s, full]) & keep) | (int(body[full]) & ~keep & 0xFF)
    twin = np.asarray(p.levels).astype(np.int8)[codes]
    return raw, twin


@pytest.mark.parametrize("bits", [1, 2, 4])
@pytest.mark.parametrize("order", ["msb", "lsb"])
def test_unpack_entry_equals_widen_on_the_twin(engines, bits, order):
    eng = engines(2_046_000)
    p = pk.offset_binary(bits, order=order)
    rng = np.random.default_rng(bits * 7 + len(order))
    for bit0 in _bit0s(p):
        for n_samples in (1, 63, 1000, 4093):
            stride = (bit0 + n_samples * p.sample_bits + 7) // 8 + int(rng.integers(1, 20))
            stride += 1 if stride % 16 == 0 else 0                        # never a multiple of 16
            raw, twin = _streams(rng, p, 3, n_samples, bit0, stride)
            d_raw = eng.alloc(raw.nbytes).upload(raw)
            out_stride = n_samples + 3
            nan = np.full(3 * out_stride, np.nan + 1j * np.nan, dtype=np.complex64)
            d_out = eng.alloc(nan.nbytes).upload(nan)
            eng.unpack_iq_dev(p, d_raw.ptr.value, 3, stride, bit0, n_samples, 0.37, out_stride, d_out.ptr.value)
            got = d_out.download(np.complex64, 3 * out_stride).reshape(3, out_stride)
            d_tw = eng.alloc(twin.nbytes).upload(np.ascontiguousarray(twin))
            d_ref = eng.alloc(twin.size * 4)
            eng.widen_iq_dev(_lib.GYP_FMT_I8, d_tw.ptr.value, twin.size, d_ref.ptr.value, 0.37)
            ref = d_ref.download(np.complex64, twin.size // 2).reshape(3, n_samples)
            for b in (d_raw, d_out, d_tw, d_ref):
                b.free()
            assert _same(got[:, :n_samples], ref), (bit0, n_samples)
            assert np.isnan(got[:, n_samples:].view(np.float32)).all()


@pytest.mark.parametrize("kind", ["resample", "ddc"])
@pytest.mark.parametrize("bits", [1, 2, 4])
@pytest.mark.parametrize("order", ["msb", "lsb"])
def test_resample_entry_equals_the_int8_entry(engines, kind, bits, order):
    fs_in, fs_out, if_hz = (2_048_000, 2_046_000, 0) if kind == "resample" else (16_368_000, 4_092_000, 4_092_000)
    eng = engines(fs_out)
    p = pk.sign_magnitude(bits, real=kind == "ddc", order=order)
    rng = np.random.default_rng(bits * 3 + len(order) + len(kind))
    n_in, n_out, n_ms = fs_in // 1000, fs_out // 1000, 3
    for bit0 in _bit0s(p):
        raw_first = int(rng.integers(-40, 40)) + n_in      # the buffer starts near millisecond 1, halo and all
        raw_n = 3 * n_in - int(rng.integers(0, 50))
        stride = (bit0 + raw_n * p.sample_bits + 7) // 8 + 5
        stride += 1 if stride % 16 == 0 else 0
        raw, twin = _streams(rng, p, 3, raw_n, bit0, stride)
        d_raw = eng.alloc(raw.nbytes).upload(raw)
        d_out = eng.alloc(3 * n_ms * n_out * 8)
        eng.resample_packed_dev(p, d_raw.ptr.value, 3, stride, bit0, raw_first, raw_n, 0.5, fs_in, if_hz, 0, 0, n_ms, n_ms * n_out,
                                d_out.ptr.value)
        got = d_out.download(np.complex64, 3 * n_ms * n_out)
        wps = p.words_per_sample
        tw = np.zeros((3, (raw_n + 7) * wps), dtype=np.int8)
        tw[:, :raw_n * wps] = twin
        d_tw = eng.alloc(tw.nbytes).upload(tw)
        d_ref = eng.alloc(3 * n_ms * n_out * 8)
        if kind == "resample":
            eng.resample_iq_dev(_lib.GYP_FMT_I8, d_tw.ptr.value, 3, raw_n + 7, raw_first, raw_n, 0.5, fs_in, 0, 0, n_ms, n_ms * n_out,
                                d_ref.ptr.value)
        else:
            eng.ddc_iq_dev(_lib.GYP_FMT_I8, d_tw.ptr.value, 3, raw_n + 7, raw_first, raw_n, 0.5, fs_in, if_hz, 0, 0, n_ms, n_ms * n_out,
                           d_ref.ptr.value)
        ref = d_ref.download(np.complex64, 3 * n_ms * n_out)
        for b in (d_raw, d_out, d_tw, d_ref):
            b.free()
        assert _same(got, ref), bit0
        assert np.abs(got).max() > 0


def test_refusals_on_the_device(engines, tmp_path):
    eng = engines(2_046_000)
    lib = eng.lib
    good = pk.sign_magnitude(2)
    real = pk.sign_magnitude(2, real=True)
    d = eng.alloc(4096)
    out = eng.alloc(4096 * 8)
    B = _lib.GYP_E_BAD_ARG
    u = lambda p, stride=64, bit0=0, n=16: lib.gyp_unpack_iq_dev(eng.ctx, _lib.ptr(p.record()), d.ptr, 1, stride, bit0, n, 1.0, n, out.ptr)
    assert u(good) == 0
    assert u(real) == B                                  # real words are not unpacked
    assert u(good, bit0=2) == B                          # 2-bit I,Q samples start at bits 0 or 4
    assert u(good, bit0=8) == B
    assert u(good, stride=7) == B                        # 16 samples of 4 bits need 8 bytes
    r = lambda p, if_hz, fs_in=2_048_000: lib.gyp_resample_packed_dev(eng.ctx, _lib.ptr(p.record()), d.ptr, 1, 4096, 0, 0, 4096, 1.0,
                                                                      fs_in, if_hz, 0, 0, 1, 2046, out.ptr)
    assert r(good, 0) == 0
    assert r(good, 1000) == B                            # I,Q with an IF
    assert r(real, 0, 16_368_000) == B                   # real without one
    assert r(good, 0, 2_046_000) == _lib.GYP_E_BAD_RATE  # the resampler's rule: fs_in != fs_out
    assert r(real, 4_092_000, 20_000_000) == _lib.GYP_E_BAD_RATE   # 8 fs_out >= fs_in fails at 2.046 Msps
    eng.sync()
    d.free()
    out.free()
    f = tmp_path / "x.bin"
    f.write_bytes(bytes(100000))
    with pytest.raises(_lib.GypsumHipError) as e:
        IqFileIngest(f, 2_046_000, engine=eng, packing=good, resample_from_hz=5_000_000)   # beyond a factor 2
    assert e.value.code == _lib.GYP_E_BAD_RATE
    with pytest.raises(ValueError):
        IqFileIngest(f, 2_046_000, engine=eng, packing=real, resample_from_hz=16_368_000)  # real without if_hz
    ing = IqFileIngest(f, 2_046_000, engine=eng, packing=good)
    with pytest.raises(_lib.GypsumHipError) as e:
        ing.next_host_block()
    assert e.value.code == B
    ing.close()


def test_batched_receiver_on_a_packed_real_if_recording(tmp_path):
    """2-bit sign-magnitude real IF at 16.368 Msps, IF 4.092 MHz: the planted satellites are acquired and tracked, and every record
    equals the int8 twin's."""
    from gypsum_amd.antenna_sample_provider import AntennaSampleProviderResampled
    from gypsum_amd.gps_ca_prn_codes import GpsSatelliteId
    from gypsum_amd.radio_input import InputFileInfo
    from gypsum_amd.receiver import BatchedGpsReceiver

    fs_in, if_hz = 16_368_000, 4_092_000
    scene = synth.random_scene(4_092_000, 700, 3, 61, max_code_phase=2046, noise_sigma=0.02)
    p = pk.sign_magnitude(2, real=True)
    info = synth.write_packed_scene(scene, fs_in, p, tmp_path / "p.bin", tmp_path / "t.bin", if_hz=if_hz)
    assert info["bytes"] * 4 == (tmp_path / "t.bin").stat().st_size
    planted = {s.sat_id for s in scene.sats}
    runs = []
    for prov in (AntennaSampleProviderResampled(InputFileInfo.packed(tmp_path / "p.bin", fs_in, p, if_hz=if_hz), resample_to=4_092_000,
                                                scale=0.03),
                 AntennaSampleProviderResampled(InputFileInfo.real_if(tmp_path / "t.bin", fs_in, if_hz, np.int8), resample_to=4_092_000,
                                                scale=0.03)):
        brx = BatchedGpsReceiver(prov, only_acquire_satellite_ids=[GpsSatelliteId(i) for i in sorted(planted | {1, 2})])
        events = brx.run(2000)
        assert brx.steps_done == prov.total_ms == 699
        runs.append((set(s.id for s in brx.tracked_satellite_ids_to_tracking_params),
                     {k.id: list(v) for k, v in brx.emitted_pseudosymbols.items()}, repr(events)))
        prov.close()
    assert runs[0][0] == planted
    assert runs[0] == runs[1]


def test_native_rate_packed_iq_recording_end_to_end(tmp_path):
    """A 2.046 Msps 2-bit I,Q recording runs at its own rate through the provider (unpack only): its planted satellites are
    acquired and tracked, and its samples equal the int8 twin's."""
    from gypsum_amd.antenna_sample_provider import AntennaSampleProviderResampled
    from gypsum_amd.gps_ca_prn_codes import GpsSatelliteId
    from gypsum_amd.radio_input import InputFileInfo
    from gypsum_amd.receiver import BatchedGpsReceiver

    fs = 2_046_000
    scene = synth.random_scene(fs, 500, 3, 17, max_code_phase=2046, noise_sigma=0.02)
    p = pk.sign_magnitude(2)
    synth.write_packed_scene(scene, fs, p, tmp_path / "p.bin", tmp_path / "t.bin")
    eng = GypsumEngine(0)
    eng.set_stream_format(fs, fs // 1000)
    twin = IqFileIngest(tmp_path / "t.bin", fs, np.int8, engine=eng, block_ms=250)
    twin.set_scale(0.03)
    _, want = _drain(eng, twin)
    twin.close()
    eng.close()
    prov = AntennaSampleProviderResampled(InputFileInfo.packed(tmp_path / "p.bin", fs, p), scale=0.03)
    assert prov.get_attributes().samples_per_second == fs
    planted = {s.sat_id for s in scene.sats}
    brx = BatchedGpsReceiver(prov, only_acquire_satellite_ids=[GpsSatelliteId(i) for i in sorted(planted | {1, 2})])
    brx.run(1000)
    assert brx.steps_done == prov.total_ms == 499
    assert {s.id for s in brx.tracked_satellite_ids_to_tracking_params} == planted
    prov.cursor = 0
    assert _same(prov.get_block(prov.total_ms).samples, want)
    prov.close()
