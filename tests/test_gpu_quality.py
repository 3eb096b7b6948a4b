"""Signal quality on the device (gyp_track_quality_dev / gyp_track_quality): the sums bit for bit against tests/quality_model.py over
window, length and bit-offset edges and over status and value edge cases; exact integer sums whatever the reduction order; the same
bits for every call shape; the argument rules; a tracked synthetic scene of known C/N0 against the float64 oracle tracker; and the
receiver's per-window figures, which must not depend on how it cuts its blocks."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import quality_model as model
from gypsum_amd import _lib, synth
from gypsum_amd import quality as ql
from gypsum_amd.engine import GypsumEngine
from oracle import gypsum_oracle as orc

pytestmark = pytest.mark.gpu

BAD = _lib.GYP_E_BAD_ARG
REC, SUMS = _lib.TRACK_REC, _lib.QUALITY_SUMS
FS, N = 2_046_000, 2046


@pytest.fixture(scope="module")
def eng():
    e = GypsumEngine(0)
    e.set_stream_format(FS, N)
    yield e
    e.close()


def _same(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _guarded(recs: np.ndarray, pad: int, lead: int):
    """(flat buffer, stride): the rows `pad` records apart beyond their length and `lead` records into the buffer; everything that
    is no row holds NaN peaks with status 0 and locked 1 -- a kernel that reads one of them shows it."""
    n_chan, n_ms = recs.shape
    stride = n_ms + pad
    flat = np.zeros(lead + n_chan * stride, dtype=REC)
    flat["peak_re"], flat["peak_im"], flat["locked"] = np.nan, np.nan, 1
    for c in range(n_chan):
        flat[lead + c * stride: lead + c * stride + n_ms] = recs[c]
    return flat, stride


def _dev_sums(eng, flat, first, n_chan, stride, n_ms, W, offs) -> np.ndarray:
    """gyp_track_quality_dev on `flat` uploaded as it is, channel 0 starting at record `first`."""
    assert first + (n_chan - 1) * stride + n_ms <= len(flat)         # the kernel reads nothing else
    n_win = -(-n_ms // W)
    d_rec = eng.alloc(flat.nbytes).upload(flat)
    d_out = eng.alloc(n_chan * n_win * SUMS.itemsize)
    eng.track_quality_dev(d_rec.ptr.value + first * REC.itemsize, n_chan, stride, n_ms, W, d_out.ptr.value, offs)
    out = d_out.download(SUMS, n_chan * n_win).reshape(n_chan, n_win)
    d_rec.free()
    d_out.free()
    return out


OFFSETS = [0, 7, -1, 19, 0]


def _edge_records(n_ms: int, seed: int) -> np.ndarray:
    """Five channels: 0 plain; 1 raises (status 1) at 2/5 of the block and is lost (2) after it; 2 plain, no bit phase; 3 lost
    throughout; 4 zero peaks in its first half (no valid group there)."""
    rng = np.random.default_rng(seed)
    peaks = (20.0 * (rng.standard_normal((5, n_ms)) + 1j * rng.standard_normal((5, n_ms))) + 15.0).astype(np.complex64)
    peaks[4, : (n_ms + 1) // 2] = 0
    rec = model.records_from_peaks(peaks, locked=rng.integers(0, 2, (5, n_ms)))
    at = (2 * n_ms) // 5
    rec["status"][1, at] = 1
    rec["status"][1, at + 1:] = 2
    rec["status"][3] = 2
    return rec


WINDOWS = [1, 20, 63, 64, 65, 250, 1000]


@pytest.mark.parametrize("n_ms", [1, 19, 20, 64, 65, 250, 1003])
def test_sums_equal_the_model_bit_for_bit(eng, n_ms):
    """Every window length against every block length, five channels at once and one of them alone, rows 3 records apart beyond
    their length: sums and counts are the model's bits."""
    rec = _edge_records(n_ms, 100 + n_ms)
    flat, stride = _guarded(rec, 3, 2)
    for W in WINDOWS:
        want = model.track_quality(rec, W, OFFSETS)
        got = _dev_sums(eng, flat, 2, 5, stride, n_ms, W, OFFSETS)
        assert _same(got, want), (W, np.flatnonzero((got != want).any(axis=1)))
        for c in (1, 4):
            one = _dev_sums(eng, flat, 2 + c * stride, 1, stride, n_ms, W, [OFFSETS[c]])
            assert _same(one[0], want[c]), (W, c)
        assert (want["reserved"] == 0).all()
        # the edge cases are in the data: a lost channel counts nothing, zero peaks make no valid group
        assert (want[3]["n_used"] == 0).all() and (want[3]["sum_p2"] == 0.0).all() and (want[3]["n_groups"] == 0).all()
        assert (want[2]["n_groups"] == 0).all() and (want[2]["sum_np"] == 0.0).all()
        assert want[1]["n_used"].sum() == (2 * n_ms) // 5 + 1
    if n_ms == 1003:
        w1000 = model.track_quality(rec, 1000, OFFSETS)
        assert w1000[0, 0]["n_groups"] == 50 and w1000[4, 0]["n_groups"] == 25      # records 0..501 are zero: the groups from 500 on have power
        assert 0 < w1000[1, 0]["n_groups"] < 50


def test_integer_peaks_sum_exactly_whatever_the_order(eng):
    """|re|, |im| < 1024: p2 < 2^21, p4 < 2^42 and every partial sum is an exact integer below 2^53, so n_used, sum_p2 and sum_p4
    equal numpy's int64 sums over the used records of each window for ANY reduction order -- a wrong item-to-record mapping shows
    even if the model repeated it."""
    rng = np.random.default_rng(5)
    n_chan, n_ms, W = 3, 1003, 250
    re, im = rng.integers(-1023, 1024, (n_chan, n_ms)), rng.integers(-1023, 1024, (n_chan, n_ms))
    status = rng.choice([0, 0, 0, 2], (n_chan, n_ms)).astype(np.int8)
    locked = rng.integers(0, 2, (n_chan, n_ms)).astype(np.int8)
    rec = model.records_from_peaks((re + 1j * im).astype(np.complex64), status=status, locked=locked)
    flat, stride = _guarded(rec, 5, 1)
    got = _dev_sums(eng, flat, 1, n_chan, stride, n_ms, W, [3, -1, 11])
    p2 = re.astype(np.int64) ** 2 + im.astype(np.int64) ** 2
    used = status != 2
    for c in range(n_chan):
        for w in range(5):
            sl = slice(w * W, min((w + 1) * W, n_ms))
            g = got[c, w]
            assert int(g["n_used"]) == int(used[c, sl].sum()) and int(g["n_locked"]) == int((used[c, sl] & (locked[c, sl] != 0)).sum())
            assert g["sum_p2"] == float(p2[c, sl][used[c, sl]].sum()) and g["sum_p4"] == float((p2[c, sl][used[c, sl]] ** 2).sum())
    assert _same(got, model.track_quality(rec, W, [3, -1, 11]))


def test_every_call_shape_gives_the_same_bits(eng):
    n_ms, W = 1003, 64
    rec = _edge_records(n_ms, 9)
    flat, stride = _guarded(rec, 7, 0)
    whole = _dev_sums(eng, flat, 0, 5, stride, n_ms, W, OFFSETS)
    for c in range(5):                                                    # one by one
        assert _same(_dev_sums(eng, flat, c * stride, 1, 0, n_ms, W, [OFFSETS[c]])[0], whole[c]), c
    packed = _dev_sums(eng, np.ascontiguousarray(rec).reshape(-1), 0, 5, n_ms, n_ms, W, OFFSETS)      # another stride
    assert _same(packed, whole)
    for w0 in (1, 5, 15):                                                 # a sub-range from record w0 W, the offsets shifted
        shifted = [b if b < 0 else (b - w0 * W) % 20 for b in OFFSETS]
        sub = _dev_sums(eng, flat, w0 * W, 5, stride, n_ms - w0 * W, W, shifted)
        assert _same(sub, whole[:, w0:]), w0
    host = eng.track_quality(rec, W, OFFSETS)                             # the host wrapper
    assert _same(host, whole)
    assert _same(eng.track_quality(rec[1], W, [OFFSETS[1]]), whole[1])
    assert _same(eng.track_quality(rec, W), model.track_quality(rec, W, None))      # NULL offsets: no groups
    # more channels than one launch's argument holds (1024): the second launch's channels and offsets line up
    many = np.ascontiguousarray(np.tile(rec[:, :40], (210, 1)))
    offs = np.tile(OFFSETS, 210)
    got = eng.track_quality(many, 20, offs)
    assert _same(got, np.tile(model.track_quality(rec[:, :40], 20, OFFSETS), (210, 1)))


def test_argument_checks(eng):
    rec = np.zeros((2, 8), dtype=REC)
    out = np.zeros((2, 2), dtype=SUMS)
    offs = np.zeros(2, dtype=np.int32)
    lib, ctx, p = eng.lib, eng.ctx, _lib.ptr
    d = eng.alloc(4096)
    dev, dev_out = C.c_void_p(d.ptr.value), C.c_void_p(d.ptr.value + 2048)      # 16 records are 896 bytes, 4 sums 192
    for fn, r, o in ((lib.gyp_track_quality, p(rec), p(out)), (lib.gyp_track_quality_dev, dev, dev_out)):
        assert fn(None, r, 2, 8, 8, 4, p(offs), o) == BAD
        assert fn(ctx, None, 2, 8, 8, 4, p(offs), o) == BAD
        assert fn(ctx, r, 2, 8, 8, 4, p(offs), None) == BAD
        assert fn(ctx, r, 0, 8, 8, 4, p(offs), o) == BAD
        assert fn(ctx, r, 2, 8, 0, 4, p(offs), o) == BAD
        assert fn(ctx, r, 2, 8, 8, 0, p(offs), o) == BAD
        assert fn(ctx, r, 2, 7, 8, 4, p(offs), o) == BAD                  # stride below n_ms with two channels
        for bad in (-2, 20):
            b = np.array([0, bad], dtype=np.int32)
            assert fn(ctx, r, 2, 8, 8, 4, p(b), o) == BAD
            assert b"bit offset" in lib.gyp_last_error(ctx)
        assert fn(ctx, r, 1, 0, 8, 4, p(offs), o) == 0                    # one channel: the stride is not read
        assert fn(ctx, r, 2, 8, 8, 4, None, o) == 0
    eng.sync()
    d.free()
    with pytest.raises(ValueError):
        eng.track_quality(rec, 4, [0])


# ---------------------------------------------------------------------------------------------------- end to end
E2E_MS, E2E_FROM, E2E_SEED = 1200, 200, 78      # (on the CPU the oracle's own figure is 0.006 dB from the scene's for this seed)
# |device - oracle| of cn0_m2m4_dbhz measured on an MI355X for this scene (profiles/quality_kernels.txt); the test allows 10 times
# that: Pn = M2 - Pd is a difference, so a relative peak error e reaches C/N0 multiplied by about twice the SNR
E2E_MEASURED_DB = 3.953e-08


def e2e_figures(eng) -> dict:
    """The end-to-end scene on the device and through the oracle (tools/quality_probe.py records the same figures)."""
    scene = synth.random_scene(FS, E2E_MS, 1, E2E_SEED)
    s = scene.sats[0]
    iq = synth.render(scene)
    t0 = np.array([orc.chunk_times(ms * N, N, FS)[0] for ms in range(E2E_MS)])
    inits = np.zeros(1, dtype=_lib.CHAN_INIT)
    inits[0] = (0, s.sat_id, float(round(s.doppler_hz)), float(s.carrier_phase), s.code_phase, 0)
    b = (-s.nav_bit_offset_ms - E2E_FROM) % 20                            # bit edges lie where (ms + nav_bit_offset_ms) % 20 == 0
    d_iq, d_t0 = eng.alloc(iq.nbytes).upload(iq), eng.alloc(t0.nbytes).upload(t0)
    d_rec, d_out = eng.alloc(E2E_MS * REC.itemsize), eng.alloc(SUMS.itemsize)
    bank = eng.create_bank(inits)
    bank.track_block_dev(d_iq.ptr.value, E2E_MS * N, E2E_MS, d_t0.ptr.value, d_rec.ptr.value)
    bank.quality_dev(d_rec.ptr.value + E2E_FROM * REC.itemsize, E2E_MS - E2E_FROM, 1000, d_out.ptr.value, [b], chan_stride=E2E_MS)
    eng.sync()
    bank.close()
    got = d_out.download(SUMS, 1)
    rec = d_rec.download(REC, E2E_MS)
    for d in (d_iq, d_t0, d_rec, d_out):
        d.free()
    q = ql.from_sums(got[0])

    trk = orc.Tracker(orc.TrackingState(float(round(s.doppler_hz)), float(s.carrier_phase), int(s.code_phase)),
                      orc.prn_as_complex(orc.generate_ca_codes()[s.sat_id - 1], N), FS, N)
    ref = np.zeros(E2E_MS, dtype=REC)
    for ms in range(E2E_MS):
        st, en = orc.chunk_times(ms * N, N, FS)
        r = trk.process_samples(iq[ms * N:(ms + 1) * N], st, en)
        ref[ms]["peak_re"], ref[ms]["peak_im"], ref[ms]["locked"] = r.peak.real, r.peak.imag, r.locked
    qo = model.from_sums(model.track_quality(ref[None, E2E_FROM:], 1000, [b])[0])
    truth = ql.cn0_of_scene(s.amplitude, scene.noise_sigma, N)
    diff = abs(q["cn0_m2m4_dbhz"] - qo["cn0_m2m4_dbhz"])
    text = (f"truth {truth:.4f} dB-Hz; device m2m4 {q['cn0_m2m4_dbhz']:.6f} nwpr {q['cn0_nwpr_dbhz']:.6f} phase_lock {q['phase_lock']:.4f}; "
            f"oracle m2m4 {qo['cn0_m2m4_dbhz']:.6f} nwpr {qo['cn0_nwpr_dbhz']:.6f}; |device - oracle| m2m4 {diff:.3e} dB")
    return {"rec": rec, "got": got, "bit_offset": b, "device": q, "oracle": qo, "truth": truth, "diff": diff, "text": text}


def test_tracked_scene_against_the_oracle_and_its_known_cn0(eng):
    """One satellite in one stream (no other code adds to the noise), tracked for 1200 ms by track_block_dev; quality_dev on the
    resident records, W = 1000 from record 200.  The sums are the model's on the downloaded records bit for bit; the device's
    C/N0 follows the float64 oracle tracker's and lies within 1 dB of what the scene was built with (a sanity cap, as on the CPU)."""
    f = e2e_figures(eng)
    print("\nquality e2e:", f["text"])
    rec, got, q, qo, truth, diff = f["rec"], f["got"], f["device"], f["oracle"], f["truth"], f["diff"]
    assert (rec["status"] == 0).all()
    assert _same(got, model.track_quality(rec[None, E2E_FROM:], 1000, [f["bit_offset"]])[0])
    assert q["n_used"] == 1000 and q["n_groups"] in (49, 50)
    assert abs(qo["cn0_m2m4_dbhz"] - truth) < 1.0                         # the oracle's records alone stay inside the cap
    assert abs(q["cn0_m2m4_dbhz"] - truth) < 1.0
    assert diff <= 10 * E2E_MEASURED_DB


# ---------------------------------------------------------------------------------------------------- receiver
def _receiver_run(iq, search, block_ms, window):
    from gypsum_amd.antenna_sample_provider import AntennaSampleProviderBackedByArray, NoMoreSamplesError
    from gypsum_amd.receiver import BatchedGpsReceiver

    kw = {} if window is None else {"quality_window_ms": window}
    rx = BatchedGpsReceiver(AntennaSampleProviderBackedByArray(iq, FS), only_acquire_satellite_ids=list(search), block_ms=block_ms, **kw)
    events = {}
    try:
        for sid, ev in rx.run(len(iq) // N).items():
            events.setdefault(sid, []).extend(ev)
    except NoMoreSamplesError:
        pass
    ev = {sid.id: [(e.receiver_timestamp, e.trailing_edge_receiver_timestamp, e.bit_value) for e in v] for sid, v in events.items()}
    sym = {sid.id: [(x.start_of_pseudosymbol, x.pseudosymbol) for x in v] for sid, v in rx.emitted_pseudosymbols.items()}
    qual = {sid.id: [(first, q.tobytes(), s.tobytes()) for first, q, s in v] for sid, v in rx.signal_quality.items()}
    return rx, ev, sym, qual


def test_receiver_quality_does_not_depend_on_the_blocks():
    from gypsum_amd.gps_ca_prn_codes import GpsSatelliteId

    scene = synth.random_scene(FS, 1300, 2, 8642, noise_sigma=0.02)
    iq = synth.render(scene)
    planted = sorted(s.sat_id for s in scene.sats)
    search = [GpsSatelliteId(s) for s in sorted(set(planted) | {1, 2})]
    rx_a, ev_a, sym_a, qual_a = _receiver_run(iq, search, 250, 200)
    rx_b, ev_b, sym_b, qual_b = _receiver_run(iq, search, 97, 200)
    rx_0, ev_0, sym_0, qual_0 = _receiver_run(iq, search, 250, None)
    assert qual_0 == {} and rx_0._quality is None
    assert ev_a == ev_b == ev_0 and sym_a == sym_b == sym_0               # the feature changes nothing the receiver returned before
    assert sorted(qual_a) == planted and qual_a == qual_b                 # same windows, bit-equal sums and figures
    truth = ql.cn0_of_scene(scene.sats[0].amplitude, scene.noise_sigma, N)
    for sid in planted:
        firsts = [f for f, _, _ in qual_a[sid]]
        assert firsts == list(range(0, 200 * len(firsts), 200)) and len(firsts) == (1300 - 9) // 200      # acquired at step 9
        qs = [np.frombuffer(q, dtype=_lib.QUALITY)[0] for _, q, _ in qual_a[sid]]
        assert all(q["n_used"] == 200 for q in qs)
        assert qs[0]["n_groups"] == 0 or len(ev_a[sid]) > 0               # groups need a decided bit
        assert qs[-1]["n_groups"] >= 9 and qs[-1]["phase_lock"] > 0.5     # by the last window the bit phase is known
        print(f"sat {sid}: truth {truth:.2f}; m2m4 {[round(float(q['cn0_m2m4_dbhz']), 2) for q in qs]}; nwpr {[round(float(q['cn0_nwpr_dbhz']), 2) for q in qs]}")
