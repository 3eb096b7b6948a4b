"""The weak-signal hand-over on the device (include/gypsum_hip.h, "weak-signal hand-over"): the prompts bit for bit against a weak
bank in SYNC and against the float64 model's sums, the estimate against tests/weak_refine_model.py and against the host twin on the
device's own prompts, bitwise invariance under the call's other candidates, their order, the stream and the stride, every refusal,
and the route search -> refine -> WeakSignalTracker from the starts on which the bank alone false-locks.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import hybrid_model as hm
import weak_refine_model as rm
import weak_track_model as wm
import weak_track_scene as ws
from gypsum_amd import _lib, _records, engine, synth
from gypsum_amd.gps_ca_prn_codes import generate_ca_code_table
from weak_shapes_scene import close_to, inits_of, results_of      # shared with tests/test_gpu_weak_shapes_*.py

pytestmark = pytest.mark.gpu

BAD_ARG = _lib.GYP_E_BAD_ARG
N_MS, FIRST_MS = 40, 7
MULTIPLES = (1, 2, 48)


def candidates(n: int):
    """(stream, satellite, candidate Doppler, true Doppler, carrier phase of the candidate, code phase, bit offset): code phase 0 with
    +10 kHz, code phase N - 1 with -10 kHz, a carrier phase a hair below zero (u0 = frac(phase / 2 pi) rounds to 1: the start rule
    makes it 0), and one in the middle -- over two streams.  The data bits alternate, so each 40-ms buffer holds two edges."""
    return [(0, 5, 10000.0, 10000.0 - 3.2, 0.7, 0, 5), (1, 9, -10000.0, -10000.0 + 4.1, -2.0, n - 1, 10), (0, 17, 1234.5, 1234.5 + 6.3, -1e-300, n // 3, 13),
            (1, 30, -250.25, -250.25 - 1.7, 3.0, n // 2 + 1, 0)]


def true_edge(bit_offset: int) -> int:
    """Millisecond i of the buffer is the absolute millisecond FIRST_MS + i and starts a bit when (i + bit_offset) % 20 == 0."""
    return (FIRST_MS - bit_offset) % 20


_cases = {}


def case(engine_factory, mult: int) -> dict:
    """One two-stream scene per rate, refined once through the host form; shared by the tests below and left unchanged."""
    if mult in _cases:
        return _cases[mult]
    n, fs = 1023 * mult, 1_023_000 * mult
    eng = engine_factory(fs, n)
    cand = candidates(n)
    a, sigma = synth.default_amplitudes(fs)
    rng = np.random.default_rng([20261021, mult])
    streams = []
    for s in (0, 1):
        sats = [synth.SyntheticSatellite(sat_id=sv, doppler_hz=true, code_phase=cp, carrier_phase=float(rng.uniform(-np.pi, np.pi)), amplitude=a,
                                         nav_bits=np.array([1, -1, 1, -1], dtype=np.int8), nav_bit_offset_ms=off)
                for stream, sv, _, true, _, cp, off in cand if stream == s]
        streams.append(hm.render(synth.SyntheticScene(fs=fs, n_ms=N_MS, sats=sats, noise_sigma=sigma, seed=100 + 2 * mult + s), code_doppler=True))
    x = np.ascontiguousarray(np.stack(streams), dtype=np.complex64)
    x.setflags(write=False)
    results = results_of([(stream, sv, f, phase, cp) for stream, sv, f, _, phase, cp, _ in cand])
    rec, prompts = eng.refine_weak(x, 2, FIRST_MS, results, want_prompts=True)
    for a_ in (results, rec, prompts):
        a_.setflags(write=False)
    _cases[mult] = dict(n=n, fs=fs, eng=eng, x=x, results=results, rec=rec, prompts=prompts)
    return _cases[mult]


# ---------------------------------------------------------------------------------------------- prompts
@pytest.mark.parametrize("mult", MULTIPLES)
def test_prompts_are_the_sync_prompts_of_a_weak_bank_bit_for_bit(engine_factory, mult):
    c = case(engine_factory, mult)
    eng, n, fs, x = c["eng"], c["n"], c["fs"], c["x"]
    bank = eng.create_weak_bank(inits_of(c["results"]), _records.WeakParams(sync_ms=N_MS), FIRST_MS)
    try:
        ms, _ = bank.track_block(x, 2, FIRST_MS, N_MS, want_periods=False)
    finally:
        bank.close()
    assert np.all(ms["phase"] == wm.SYNC) and np.all(ms["status"] == 0)
    want = np.stack([ms["prompt_re"], ms["prompt_im"]], axis=-1)
    assert want.dtype == np.float32 and c["prompts"].shape == (4, N_MS)
    assert c["prompts"].view(np.float32).reshape(4, N_MS, 2).tobytes() == want.tobytes()
    assert np.count_nonzero(c["prompts"]) == 4 * N_MS
    # and the model's sums: the project's 1e-4 ||x_ms||_2 bar
    chips = generate_ca_code_table().astype(np.float64) * 2 - 1
    worst = 0.0
    for i, r in enumerate(c["results"]):
        model = rm.open_loop_sums(x[int(r["stream"])], chips[int(r["sat_id"]) - 1], fs, n, float(r["doppler_hz"]), float(r["carrier_phase"]),
                                     int(r["code_phase"]), N_MS)
        for m in range(N_MS):
            norm = float(np.linalg.norm(x[int(r["stream"]), m * n:(m + 1) * n].astype(np.complex128)))
            err = abs(complex(c["prompts"][i, m]) - complex(model[m]))
            worst = max(worst, err / norm)
            assert err <= 1e-4 * norm, (mult, i, m, err, norm)
    assert wm.init_u0(float(c["results"][2]["carrier_phase"])) == 0.0                                     # the hair below zero
    print(f"{fs} Hz: largest |device - model| / ||x_ms||_2 = {worst:.3g}")


@pytest.mark.parametrize("mult", MULTIPLES)
def test_records_are_the_models_estimate_on_the_devices_prompts(engine_factory, mult):
    c = case(engine_factory, mult)
    for i, (r, got) in enumerate(zip(c["results"], c["rec"])):
        want = rm.estimate(c["prompts"][i], FIRST_MS)
        k, P = want.bin, want.power
        assert all(P[k] > P[j] * (1 + 1e-9) for j in (k - 1, k + 1) if 0 <= j < len(P))          # on the model alone: no tie to break
        print(f"{c['fs']} Hz result {i}: delta {float(got['delta_hz']):+.6f} (model {want.delta_hz:+.6f}), truth {candidates(c['n'])[i][3] - candidates(c['n'])[i][2]:+.1f}; "
              f"peak/mean {float(got['peak_to_mean']):.2f}, edge {int(got['edge'])}, ratio {float(got['edge_ratio']):.4f}")
        close_to(got, want, float(r["doppler_hz"]), float(r["carrier_phase"]))
        assert (int(got["stream"]), int(got["sat_id"]), int(got["code_phase"])) == (int(r["stream"]), int(r["sat_id"]), int(r["code_phase"]))
        assert int(got["status"]) == 0 and int(got["edge"]) == true_edge(candidates(c["n"])[i][6])
        # peak_to_mean: with 81 bins and a guard of ceil(1000 / (40 * 0.5)) = 50 only a peak more than 10 bins off the centre has a far bin
        assert math.isnan(float(got["peak_to_mean"])) == (abs(int(got["bin"]) - 40) <= 10)
        # 40 ms of a strong signal: the main lobe is 25 Hz wide and the estimate lands within 1.5 Hz of the residual put in
        assert abs(float(got["doppler_hz"]) - candidates(c["n"])[i][3]) < 1.5


@pytest.mark.parametrize("mult", MULTIPLES)
def test_host_twin_agrees_with_the_device_on_its_prompts(engine_factory, mult):
    c = case(engine_factory, mult)
    for i, (r, got) in enumerate(zip(c["results"], c["rec"])):
        twin = engine.weak_refine_estimate(c["prompts"][i], FIRST_MS)
        as_model = rm.Refined(float(twin["delta_hz"]), float(twin["carrier_phase"]), int(twin["edge"]), float(twin["peak_to_mean"]),
                              float(twin["edge_ratio"]), int(twin["bin"]), int(twin["status"]), None, None)
        close_to(got, as_model, float(r["doppler_hz"]), float(r["carrier_phase"]))


# ---------------------------------------------------------------------------------------------- invariance
def test_a_result_does_not_depend_on_the_calls_other_results_their_order_the_stream_or_the_stride(engine_factory):
    c = case(engine_factory, 2)
    eng, n, x, res = c["eng"], c["n"], c["x"], c["results"]
    twice = np.ascontiguousarray(np.stack([x[0], x[0]]))                    # both streams hold stream 0's samples
    mine = res[2:3].copy()                                                  # a candidate of stream 0
    on_1 = mine.copy()
    on_1["stream"] = 1

    def same(rec, prompts, stream=0):
        want = c["rec"][2:3].copy()
        want["stream"] = stream
        assert rec.tobytes() == want.tobytes() and prompts.tobytes() == c["prompts"][2:3].tobytes()

    rec, p = eng.refine_weak(x[0], 1, FIRST_MS, mine, want_prompts=True)                    # alone, on a one-stream call
    same(rec, p)
    rec, p = eng.refine_weak(x, 2, FIRST_MS, np.concatenate([mine, res[:2], res[3:]]), want_prompts=True)      # first
    same(rec[:1], p[:1])
    rec, p = eng.refine_weak(x, 2, FIRST_MS, np.concatenate([res[3:], res[:2], res[:2], mine]), want_prompts=True)      # last of six
    same(rec[-1:], p[-1:])
    assert rec[1:3].tobytes() == rec[3:5].tobytes() == c["rec"][:2].tobytes()               # (and a result given twice is two equal records)
    rec, p = eng.refine_weak(twice, 2, FIRST_MS, np.concatenate([mine, on_1]), want_prompts=True)
    same(rec[:1], p[:1])
    same(rec[1:], p[1:], stream=1)
    # the device form, the streams a stride larger than n_ms N apart
    stride = N_MS * n + 77
    wide = np.zeros(2 * stride, dtype=np.complex64)
    wide[:N_MS * n], wide[stride:stride + N_MS * n] = x[0], x[1]
    d_iq = eng.alloc(wide.nbytes).upload(wide)
    d_out, d_p = eng.alloc(4 * _lib.WEAK_REFINED.itemsize), eng.alloc(4 * N_MS * 8)
    try:
        eng.refine_weak_dev(d_iq.ptr.value, 2, stride, FIRST_MS, N_MS, res, d_out.ptr.value, None, d_p.ptr.value)
        eng.sync()
        assert d_out.download(_lib.WEAK_REFINED, 4).tobytes() == c["rec"].tobytes()
        assert d_p.download(np.complex64, 4 * N_MS).tobytes() == c["prompts"].tobytes()
        eng.refine_weak_dev(d_iq.ptr.value, 2, stride, FIRST_MS, N_MS, res, d_out.ptr.value)      # and without the prompts
        eng.sync()
        assert d_out.download(_lib.WEAK_REFINED, 4).tobytes() == c["rec"].tobytes()
    finally:
        for b in (d_iq, d_out, d_p):
            b.free()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing_and_leave_the_context_usable(engine_factory):
    c = case(engine_factory, 2)
    eng, n, res = c["eng"], c["n"], c["results"]
    lib, ctx, p = eng.lib, eng.ctx, _lib.ptr
    x = np.ascontiguousarray(c["x"]).reshape(-1)
    out = np.full(4 * 64, 7, dtype=np.uint8)
    prompts = np.full(4 * N_MS * 2, 7.0, dtype=np.float32)
    d_iq = eng.alloc(x.nbytes).upload(x)
    d_out = eng.alloc(out.nbytes).upload(out)

    def prm(**kw):
        return _records.WeakRefineParams(**kw).record()

    def host(iq=x, n_streams=2, first=FIRST_MS, n_ms=N_MS, results=res, n_results=4, params=None, o=out):
        return lib.gyp_weak_refine(ctx, None if iq is None else p(iq), n_streams, first, n_ms, None if results is None else p(results), n_results, p(params),
                                   None if o is None else p(o), p(prompts))

    def dev(iq=d_iq.ptr, n_streams=2, stride=N_MS * n, first=FIRST_MS, n_ms=N_MS, results=res, n_results=4, params=None, o=d_out.ptr):
        return lib.gyp_weak_refine_dev(ctx, iq, n_streams, stride, first, n_ms, None if results is None else p(results), n_results, p(params), o, None)

    def res_with(i=1, **kw):
        a = res.copy()
        for k, v in kw.items():
            a[k][i] = v
        return a

    refusals = []
    for name, call in (("host", host), ("dev", dev)):
        refusals += [(name, what, (lambda c=call, k=kw: c(**k))) for what, kw in (
            ("span 0", dict(params=prm(span_hz=0.0))), ("span above 100", dict(params=prm(span_hz=100.5, presum_ms=1))), ("span NaN", dict(params=prm(span_hz=float("nan")))),
            ("step below 0.01", dict(params=prm(step_hz=0.009))), ("step above the span", dict(params=prm(step_hz=20.5))), ("step NaN", dict(params=prm(step_hz=float("nan")))),
            ("presum 3", dict(params=prm(presum_ms=3))), ("presum 0", dict(params=prm(presum_ms=0))), ("presum 40", dict(params=prm(presum_ms=40))),
            ("span at 250 / presum", dict(params=prm(span_hz=62.5))), ("span at 250 / presum, presum 20", dict(params=prm(span_hz=12.5, presum_ms=20))),
            ("4099 bins", dict(params=prm(span_hz=20.5, step_hz=0.01))),
            ("n_ms 39", dict(n_ms=39)), ("n_ms 2001", dict(n_ms=2001)), ("n_ms 0", dict(n_ms=0)), ("two groups of twenty", dict(params=prm(presum_ms=20, span_hz=10.0))),
            ("four groups of ten", dict(params=prm(presum_ms=10, span_hz=10.0))), ("first_ms < 0", dict(first=-1)),
            ("NULL samples", dict(iq=None)), ("NULL results", dict(results=None)), ("NULL out", dict(o=None)),
            ("no results", dict(n_results=0)), ("a negative count", dict(n_results=-1)), ("no streams", dict(n_streams=0)),
            ("a negative stream", dict(results=res_with(stream=-1))), ("a stream that was not passed", dict(results=res_with(stream=2))),
            ("stream 1 of one", dict(n_streams=1)), ("satellite 0", dict(results=res_with(sat_id=0))), ("satellite 33", dict(results=res_with(sat_id=33))),
            ("a NaN Doppler", dict(results=res_with(doppler_hz=np.nan))), ("an infinite Doppler", dict(results=res_with(i=3, doppler_hz=np.inf))),
            ("a NaN carrier phase", dict(results=res_with(carrier_phase=np.nan))), ("code phase -1", dict(results=res_with(code_phase=-1))),
            ("code phase N", dict(results=res_with(i=0, code_phase=n))))]
    refusals += [("dev", "a stride below n_ms N", lambda: dev(stride=N_MS * n - 1)), ("dev", "a negative stride", lambda: dev(stride=-1))]
    try:
        for name, what, call in refusals:
            assert call() == BAD_ARG, (name, what)
            assert lib.gyp_last_error(ctx), (name, what)
        eng.sync()
        assert np.all(out == 7) and np.all(prompts == 7.0) and np.all(d_out.download(np.uint8, out.size) == 7)      # nothing ran, nothing was written
        assert host(params=prm(span_hz=20.48, step_hz=0.01)) == 0                                                     # 4097 bins are taken
        # and the context still gives the known answer, through both forms
        assert host() == 0 and dev() == 0
        eng.sync()
        assert out.tobytes() == c["rec"].tobytes() and prompts.tobytes() == c["prompts"].tobytes()
        assert d_out.download(_lib.WEAK_REFINED, 4).tobytes() == c["rec"].tobytes()
    finally:
        d_iq.free()
        d_out.free()


# ---------------------------------------------------------------------------------------------- the route
def test_search_refine_tracker_gives_the_bits_from_the_farther_search_bin():
    """The counterpart of test_gpu_weak_track.py::test_false_lock_from_the_farther_search_bin_is_flagged: the same starts -- the
    search's farther fine bin, 7 and 8 Hz off, the code phase the search found, carrier phase 0.3 -- refined on the search's 220 ms
    first, then tracked: every bit, no false lock."""
    from gypsum_amd.acquisition import GpsSatelliteDetector, SatelliteAcquisitionAttemptResult
    from gypsum_amd.antenna_sample_provider import SampleProviderAttributes
    from gypsum_amd.tracker import BitValue
    from gypsum_amd.weak_tracker import WeakSignalTracker
    attrs = SampleProviderAttributes(samples_per_second=ws.FS, samples_per_prn_transmission=ws.N)
    x, tr, g = ws.iq(), ws.truth(), ws.golden()
    assert tuple(g["search_sat"]) == tuple(sv for sv, _ in ws.FAR_BIN_STARTS)
    starts = [SatelliteAcquisitionAttemptResult(satellite_id=sv, doppler_shift=f, carrier_wave_phase_shift=0.3, prn_phase_shift=int(g["search_code_phase"][i]),
                                                correlation_strength=30.0) for i, (sv, f) in enumerate(ws.FAR_BIN_STARTS)]
    refined = GpsSatelliteDetector({}).refine_weak_satellites(starts, x[:ws.SEARCH_MS * ws.N], attrs)
    assert [r.satellite_id for r in refined] == [s.satellite_id for s in starts]                  # it drops nothing
    for s, r in zip(starts, refined):
        sat = tr[s.satellite_id]
        print(f"satellite {s.satellite_id}: {s.doppler_shift - sat.doppler_hz:+.0f} Hz -> {r.doppler_shift - sat.doppler_hz:+.3f} Hz off")
        assert abs(s.doppler_shift - sat.doppler_hz) >= 7.0 and abs(r.doppler_shift - sat.doppler_hz) <= 1.0
        assert r.prn_phase_shift == s.prn_phase_shift and r.correlation_strength == s.correlation_strength
    trk = WeakSignalTracker(refined, attrs)
    events = trk.process(x)
    for c, s in enumerate(starts):
        sat = tr[s.satellite_id]
        ev = [e for ch, e in events if ch == c]
        first = [round(e.receiver_timestamp * 1000) for e in ev]
        assert len(ev) >= 99 and first[0] % 20 == ws.true_edge(sat)
        got = [1 if e.bit_value == BitValue.ONE else -1 for e in ev][ws.SETTLE_PERIODS:]
        want = [ws.true_bit(sat, m) for m in first][ws.SETTLE_PERIODS:]
        same = sum(int(a == b) for a, b in zip(got, want))
        assert same in (0, len(want)), (s.satellite_id, same, len(want))                          # every bit, up to the one sign
    for s, st in zip(starts, trk.status()):
        print(f"satellite {s.satellite_id}: mu {st.mu:.2f} phase rms {st.phase_rms:.3f}")
        assert st.status == 0 and not st.false_lock and st.phase_rms < 0.5 and st.bit_edge == ws.true_edge(tr[s.satellite_id])
