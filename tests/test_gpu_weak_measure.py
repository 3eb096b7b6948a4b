"""The weak-signal measurement on the device (include/gypsum_hip.h, "weak-signal measurement"): each pass's sums bit for bit against a
weak bank (in SYNC for pass 1, put at the corrected c0 through set_state for pass 2) and W_m against numpy, each pass's fold against
the host twin on the device's own sums -- bit for bit: the build has no fast-math flag, so the device's float64 division and square
root are the correctly rounded ones -- the record against tests/weak_measure_model.py on the device's input, bitwise invariance under
the call's other candidates, their order, the stream and the stride, every refusal, all-zero samples, and the route
search -> measure -> WeakSignalTracker.from_measurements on a 30 dB-Hz scene with fractional code phases.

Measured on an MI355X (printed by the parity test): the record against the float64 model on the device's input, over 1.023, 2.046
and 49.104 Msps and twelve candidates, differs by at most 1.1e-8 chip in c0 and 7.9e-8 dB in the C/N0 -- the bars are 1e-4 chip and 1e-3 dB.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import weak_measure_model as mm
import weak_track_model as wm
from gypsum_amd import _lib, _records, engine, synth
from weak_shapes_scene import inits_of, refined_of      # shared with tests/test_gpu_weak_shapes_*.py

pytestmark = pytest.mark.gpu

BAD_ARG = _lib.GYP_E_BAD_ARG
N_MS, FIRST_MS = 40, 7
MULTIPLES = (1, 2, 48)
#          passes  spacing
SETTINGS = ((2, 1 << 39), (4, 1 << 36), (1, 1 << 38))
SIX = ("minus_re", "minus_im", "prompt_re", "prompt_im", "plus_re", "plus_im")


def candidates(n: int):
    """(stream, satellite, Doppler, carrier phase of the candidate, integer code phase, the fraction added to it in the scene, bit
    offset): code phase 0 with +10 kHz, code phase N - 1 with -10 kHz, a carrier phase a hair below zero, and one in the middle --
    over two streams.  The data bits alternate, so each 40-ms buffer holds two edges."""
    return [(0, 5, 10000.0, 0.7, 0, 0.31, 5), (1, 9, -10000.0, -2.0, n - 1, -0.42, 10), (0, 17, 1234.5, -1e-300, n // 3, 0.18, 13),
            (1, 30, -250.25, 3.0, n // 2 + 1, -0.07, 0)]


def true_edge(bit_offset: int) -> int:
    """Millisecond i of the buffer is the absolute millisecond FIRST_MS + i and starts a bit when (i + bit_offset) % 20 == 0."""
    return (FIRST_MS - bit_offset) % 20


def prm(passes: int, spacing: int) -> _records.WeakMeasureParams:
    return _records.WeakMeasureParams(spacing=spacing, passes=passes)


_cases = {}


def case(engine_factory, mult: int) -> dict:
    """One two-stream scene per rate, measured once per setting through the host form; shared by the tests below and left unchanged."""
    if mult in _cases:
        return _cases[mult]
    n, fs = 1023 * mult, 1_023_000 * mult
    eng = engine_factory(fs, n)
    cand = candidates(n)
    a, sigma = synth.default_amplitudes(fs)
    rng = np.random.default_rng([20261021, mult])
    streams = []
    for s in (0, 1):
        sats = [mm.Sat(sv, f, cp + frac, float(rng.uniform(-np.pi, np.pi)), a, np.array([1, -1, 1, -1], dtype=np.int8), off)
                for stream, sv, f, _, cp, frac, off in cand if stream == s]
        streams.append(mm.render(sats, fs, n, N_MS, sigma, 300 + 2 * mult + s))
    x = np.ascontiguousarray(np.stack(streams), dtype=np.complex64)
    x.setflags(write=False)
    refined = refined_of([(stream, sv, f, phase, cp, true_edge(off)) for stream, sv, f, phase, cp, _, off in cand])
    runs = {}
    for passes, spacing in SETTINGS:
        runs[(passes, spacing)] = eng.measure_weak(x, 2, FIRST_MS, refined, prm(passes, spacing), want_sums=True)
        for a_ in runs[(passes, spacing)]:
            a_.setflags(write=False)
    refined.setflags(write=False)
    _cases[mult] = dict(n=n, fs=fs, eng=eng, x=x, refined=refined, runs=runs)
    return _cases[mult]


# ---------------------------------------------------------------------------------------------- sums
@pytest.mark.parametrize("mult", MULTIPLES)
def test_sums_are_a_weak_banks_bit_for_bit(engine_factory, mult):
    c = case(engine_factory, mult)
    eng, n, fs, x, refined = c["eng"], c["n"], c["fs"], c["x"], c["refined"]
    for (passes, spacing), (rec, sums, w, folds) in c["runs"].items():
        assert sums.shape == w.shape == (4, passes, N_MS) and folds.shape == (4, passes)
        # pass 1: the SYNC records of a bank created from the candidates with this spacing, every field
        bank = eng.create_weak_bank(inits_of(refined), _records.WeakParams(sync_ms=N_MS, spacing=spacing), FIRST_MS)
        try:
            ms, _ = bank.track_block(x, 2, FIRST_MS, N_MS, want_periods=False)
        finally:
            bank.close()
        assert np.all(ms["phase"] == wm.SYNC) and np.all(ms["status"] == 0)
        assert sums[:, 0, :].tobytes() == ms.tobytes(), (mult, passes, spacing)
        assert all(np.count_nonzero(sums[:, 0, :][k]) == 4 * N_MS for k in SIX)
        # W_m against numpy float64
        for i, r in enumerate(refined):
            xs = x[int(r["stream"])].reshape(N_MS, n).astype(np.complex128)
            want = np.sum(xs.real * xs.real + xs.imag * xs.imag, axis=1)
            for p in range(passes):
                assert np.all(np.abs(w[i, p] - want) <= 1e-12 * want), (mult, i, p)
                assert w[i, p].tobytes() == w[i, 0].tobytes()                     # (and the same bits in every pass)
        if passes < 2:
            continue
        # pass 2: a bank put at the corrected c0 through set_state, waiting: 19 ms at a time with the edge kept 19 ms ahead, the state
        # advanced by gyp_weak_measured_state
        bank = eng.create_weak_bank(inits_of(refined), _records.WeakParams(sync_ms=N_MS, spacing=spacing), FIRST_MS)
        got = np.zeros((4, N_MS), dtype=_lib.WEAK_MS_REC)
        try:
            for at in range(0, N_MS, 19):
                for i in range(4):
                    start = rec[i:i + 1].copy()
                    start["c0"], start["edge"] = folds[i, 0]["c0"], (FIRST_MS + at + 19) % 20
                    st = engine.weak_measured_state(start, fs, n, at)
                    bank.set_state(i, float(st["f"]), float(st["f_int"]), float(st["u0"]), int(st["c0"]), int(st["edge"]))
                k = min(19, N_MS - at)
                ms, _ = bank.track_block(np.ascontiguousarray(x[:, at * n:(at + k) * n]), 2, FIRST_MS + at, k, want_periods=False)
                assert np.all(ms["phase"] == wm.WAIT)
                got[:, at:at + k] = ms
        finally:
            bank.close()
        for k in SIX:
            assert sums[:, 1, :][k].tobytes() == got[k].tobytes(), (mult, passes, spacing, k)
        # the correction moved the replica; on the sample lattice that changes a sum only where some sample's chip changes: with 48
        # samples per chip and 12 samples of code drift it does; at one or two samples per chip a correction below the grid's step may
        # change none, and with d = 1/16 chip the three replicas are one and the same there (dd = 0)
        if mult == 48:
            assert all(sums[:, 1, :][k].tobytes() != sums[:, 0, :][k].tobytes() for k in SIX)


# ---------------------------------------------------------------------------------------------- passes
@pytest.mark.parametrize("mult", MULTIPLES)
def test_every_pass_is_the_twins_fold_of_the_devices_sums(engine_factory, mult):
    c = case(engine_factory, mult)
    n = c["n"]
    for (passes, spacing), (rec, sums, w, folds) in c["runs"].items():
        for i, r in enumerate(c["refined"]):
            c0 = wm.init_c0(int(r["code_phase"]), n)
            delta, status = 0.0, 0
            for p in range(passes):
                twin = engine.weak_measure_estimate(sums[i, p], w[i, p], FIRST_MS, int(r["edge"]), c0, spacing)
                got = folds[i, p]
                for name in ("e_minus", "e_prompt", "e_plus", "wn", "dd", "c0", "n_groups", "status"):
                    assert got[name] == twin[name], (mult, passes, spacing, i, p, name, got[name], twin[name])        # bit for bit
                assert abs(float(got["cn0_dbhz"]) - float(twin["cn0_dbhz"])) <= 1e-9
                assert int(got["c0"]) == (c0 + wm.llround(float(got["dd"]) * wm.ONE)) % wm.CODE_MOD
                c0, delta, status = int(got["c0"]), delta + float(got["dd"]), status | int(got["status"])
            o = rec[i]
            print(f"{c['fs']} Hz passes {passes} spacing 2^{spacing.bit_length() - 1} candidate {i}: dd {[round(float(f['dd']), 5) for f in folds[i]]} "
                  f"code phase {float(o['code_phase_samples']):.4f} (scene {candidates(n)[i][4] + candidates(n)[i][5]:.2f}) cn0 {float(o['cn0_dbhz']):.2f}")
            assert (int(o["c0"]), float(o["delta_chips"]), float(o["dd_last"]), int(o["status"])) == (c0, delta, float(folds[i, -1]["dd"]), status)
            assert float(o["cn0_dbhz"]) == float(folds[i, -1]["cn0_dbhz"]) and float(o["code_phase_samples"]) == mm.code_phase_samples(c0, n)
            assert (int(o["stream"]), int(o["sat_id"]), float(o["doppler_hz"]), float(o["carrier_phase"]), int(o["edge"]), int(o["reserved"])) == \
                (int(r["stream"]), int(r["sat_id"]), float(r["doppler_hz"]), float(r["carrier_phase"]), int(r["edge"]), 0)
            assert int(o["n_groups"]) == mm.n_groups(N_MS, FIRST_MS, int(r["edge"])) == (1 if int(r["edge"]) != FIRST_MS % 20 else 2)
            assert int(o["status"]) == 0


# ---------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("mult", MULTIPLES)
def test_records_are_the_models_on_the_devices_input(engine_factory, mult):
    c = case(engine_factory, mult)
    n, fs, x = c["n"], c["fs"], c["x"]
    rec = c["runs"][(2, 1 << 39)][0]
    worst_c0 = worst_cn0 = 0.0
    for i, r in enumerate(c["refined"]):
        m = mm.measure(x[int(r["stream"])], mm.chips_pm(int(r["sat_id"])), fs, n, float(r["doppler_hz"]), float(r["carrier_phase"]), int(r["code_phase"]),
                       int(r["edge"]), FIRST_MS, N_MS)
        d_c0 = abs((int(rec[i]["c0"]) - m.c0 + wm.CODE_MOD // 2) % wm.CODE_MOD - wm.CODE_MOD // 2) / wm.ONE
        d_cn0 = abs(float(rec[i]["cn0_dbhz"]) - m.cn0_dbhz)
        worst_c0, worst_cn0 = max(worst_c0, d_c0), max(worst_cn0, d_cn0)
        print(f"{fs} Hz candidate {i}: |c0 - model| {d_c0:.3g} chip, |cn0 - model| {d_cn0:.3g} dB (cn0 {float(rec[i]['cn0_dbhz']):.3f})")
        assert d_c0 <= 1e-4 and d_cn0 <= 1e-3, (mult, i, d_c0, d_cn0)
        assert abs(float(rec[i]["delta_chips"]) - m.delta_chips) <= 1e-4 and abs(float(rec[i]["dd_last"]) - m.dd_last) <= 1e-4
        assert (int(rec[i]["n_groups"]), int(rec[i]["status"])) == (m.n_groups, m.status)
    print(f"{fs} Hz: largest |device - model|: {worst_c0:.3g} chip, {worst_cn0:.3g} dB")


# ---------------------------------------------------------------------------------------------- invariance
def test_a_record_does_not_depend_on_the_calls_other_candidates_their_order_the_stream_or_the_stride(engine_factory):
    c = case(engine_factory, 2)
    eng, n, x, ref = c["eng"], c["n"], c["x"], c["refined"]
    passes, spacing = 2, 1 << 39
    known = c["runs"][(passes, spacing)]
    twice = np.ascontiguousarray(np.stack([x[0], x[0]]))                    # both streams hold stream 0's samples
    mine = ref[2:3].copy()                                                  # a candidate of stream 0
    on_1 = mine.copy()
    on_1["stream"] = 1

    def same(got, at, stream=0):
        want = known[0][2:3].copy()
        want["stream"] = stream
        assert got[0][at:at + 1].tobytes() == want.tobytes()
        for g, k in zip(got[1:], known[1:]):
            assert g[at:at + 1].tobytes() == k[2:3].tobytes()

    same(eng.measure_weak(x[0], 1, FIRST_MS, mine, want_sums=True), 0)                                          # alone, on a one-stream call
    same(eng.measure_weak(x, 2, FIRST_MS, np.concatenate([mine, ref[:2], ref[3:]]), want_sums=True), 0)        # first
    got = eng.measure_weak(x, 2, FIRST_MS, np.concatenate([ref[3:], ref[:2], ref[:2], mine]), want_sums=True)  # last of six
    same(got, 5)
    assert got[0][1:3].tobytes() == got[0][3:5].tobytes() == known[0][:2].tobytes()                            # (a candidate given twice: two equal records)
    got = eng.measure_weak(twice, 2, FIRST_MS, np.concatenate([mine, on_1]), want_sums=True)
    same(got, 0)
    same(got, 1, stream=1)
    assert eng.measure_weak(x, 2, FIRST_MS, ref)[0].tobytes() == known[0].tobytes()                            # without the sums: scratch rows
    # the device form, the streams a stride larger than n_ms N apart
    stride = N_MS * n + 77
    wide = np.zeros(2 * stride, dtype=np.complex64)
    wide[:N_MS * n], wide[stride:stride + N_MS * n] = x[0], x[1]
    rows = 4 * passes * N_MS
    d_iq = eng.alloc(wide.nbytes).upload(wide)
    d_out, d_sums, d_w = eng.alloc(4 * _lib.WEAK_MEASURED.itemsize), eng.alloc(rows * _lib.WEAK_MS_REC.itemsize), eng.alloc(rows * 8)
    d_folds = eng.alloc(4 * passes * _lib.WEAK_MEASURE_FOLD.itemsize)
    try:
        eng.measure_weak_dev(d_iq.ptr.value, 2, stride, FIRST_MS, N_MS, ref, d_out.ptr.value, None, d_sums.ptr.value, d_w.ptr.value, d_folds.ptr.value)
        eng.sync()
        assert d_out.download(_lib.WEAK_MEASURED, 4).tobytes() == known[0].tobytes()
        assert d_sums.download(_lib.WEAK_MS_REC, rows).tobytes() == known[1].tobytes()
        assert d_w.download(np.float64, rows).tobytes() == known[2].tobytes()
        assert d_folds.download(_lib.WEAK_MEASURE_FOLD, 4 * passes).tobytes() == known[3].tobytes()
        d_out.upload(np.zeros(4 * _lib.WEAK_MEASURED.itemsize, dtype=np.uint8))
        eng.measure_weak_dev(d_iq.ptr.value, 2, stride, FIRST_MS, N_MS, ref, d_out.ptr.value, None, 0, d_w.ptr.value)      # the sums in scratch, the W_m not
        eng.sync()
        assert d_out.download(_lib.WEAK_MEASURED, 4).tobytes() == known[0].tobytes()
    finally:
        for b in (d_iq, d_out, d_sums, d_w, d_folds):
            b.free()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing_and_leave_the_context_usable(engine_factory):
    c = case(engine_factory, 2)
    eng, n, ref = c["eng"], c["n"], c["refined"]
    known = c["runs"][(2, 1 << 39)]
    lib, ctx, p = eng.lib, eng.ctx, _lib.ptr
    x = np.ascontiguousarray(c["x"]).reshape(-1)
    out = np.full(4 * 80, 7, dtype=np.uint8)
    sums = np.full(4 * 2 * N_MS * 32, 7, dtype=np.uint8)
    d_iq = eng.alloc(x.nbytes).upload(x)
    d_out = eng.alloc(out.nbytes).upload(out)

    def params(**kw):
        return _records.WeakMeasureParams(**kw).record()

    def host(iq=x, n_streams=2, first=FIRST_MS, n_ms=N_MS, refined=ref, n_results=4, prm_=None, o=out):
        return lib.gyp_weak_measure(ctx, None if iq is None else p(iq), n_streams, first, n_ms, None if refined is None else p(refined), n_results, p(prm_),
                                    None if o is None else p(o), p(sums), None, None)

    def dev(iq=d_iq.ptr, n_streams=2, stride=N_MS * n, first=FIRST_MS, n_ms=N_MS, refined=ref, n_results=4, prm_=None, o=d_out.ptr):
        return lib.gyp_weak_measure_dev(ctx, iq, n_streams, stride, first, n_ms, None if refined is None else p(refined), n_results, p(prm_), o, None, None, None)

    def ref_with(i=1, **kw):
        a = ref.copy()
        for k, v in kw.items():
            a[k][i] = v
        return a

    refusals = []
    for name, call in (("host", host), ("dev", dev)):
        refusals += [(name, what, (lambda c=call, k=kw: c(**k))) for what, kw in (
            ("spacing below 2^36", dict(prm_=params(spacing=(1 << 36) - 1))), ("spacing above 2^39", dict(prm_=params(spacing=(1 << 39) + 1))),
            ("spacing 0", dict(prm_=params(spacing=0))), ("a negative spacing", dict(prm_=params(spacing=-(1 << 38)))),
            ("no pass", dict(prm_=params(passes=0))), ("five passes", dict(prm_=params(passes=5))),
            ("n_ms 39", dict(n_ms=39)), ("n_ms 2001", dict(n_ms=2001)), ("n_ms 0", dict(n_ms=0)), ("first_ms < 0", dict(first=-1)),
            ("NULL samples", dict(iq=None)), ("NULL candidates", dict(refined=None)), ("NULL out", dict(o=None)),
            ("no candidates", dict(n_results=0)), ("a negative count", dict(n_results=-1)), ("no streams", dict(n_streams=0)),
            ("a negative stream", dict(refined=ref_with(stream=-1))), ("a stream that was not passed", dict(refined=ref_with(stream=2))),
            ("stream 1 of one", dict(n_streams=1)), ("satellite 0", dict(refined=ref_with(sat_id=0))), ("satellite 33", dict(refined=ref_with(sat_id=33))),
            ("a NaN Doppler", dict(refined=ref_with(doppler_hz=np.nan))), ("an infinite Doppler", dict(refined=ref_with(i=3, doppler_hz=np.inf))),
            ("a NaN carrier phase", dict(refined=ref_with(carrier_phase=np.nan))), ("code phase -1", dict(refined=ref_with(code_phase=-1))),
            ("code phase N", dict(refined=ref_with(i=0, code_phase=n))), ("edge -1", dict(refined=ref_with(edge=-1))),
            ("edge 20", dict(refined=ref_with(i=3, edge=20))))]
    refusals += [("dev", "a stride below n_ms N", lambda: dev(stride=N_MS * n - 1)), ("dev", "a negative stride", lambda: dev(stride=-1))]
    try:
        for name, what, call in refusals:
            assert call() == BAD_ARG, (name, what)
            assert lib.gyp_last_error(ctx), (name, what)
        eng.sync()
        assert np.all(out == 7) and np.all(sums == 7) and np.all(d_out.download(np.uint8, out.size) == 7)      # nothing ran, nothing was written
        # and the context still gives the known answer, through both forms
        assert host() == 0 and dev() == 0
        eng.sync()
        assert out.tobytes() == known[0].tobytes() and sums.tobytes() == known[1].tobytes()
        assert d_out.download(_lib.WEAK_MEASURED, 4).tobytes() == known[0].tobytes()
    finally:
        d_iq.free()
        d_out.free()


def test_all_zero_samples_give_status_bit_1(engine_factory):
    c = case(engine_factory, 2)
    eng, n, ref = c["eng"], c["n"], c["refined"]
    rec, sums, w, folds = eng.measure_weak(np.zeros(2 * N_MS * n, dtype=np.complex64), 2, FIRST_MS, ref, prm(3, 1 << 39), want_sums=True)
    assert np.all(rec["status"] == 1) and np.all(folds["status"] == 1) and np.all(np.isnan(rec["cn0_dbhz"])) and np.all(w == 0.0)
    assert all(np.all(sums[k] == 0.0) for k in SIX)
    assert np.all(rec["delta_chips"] == 0.0) and np.all(rec["dd_last"] == 0.0)
    assert [int(v) for v in rec["c0"]] == [wm.init_c0(int(r["code_phase"]), n) for r in ref]                 # c0 is the start
    assert [float(v) for v in rec["code_phase_samples"]] == [float(r["code_phase"]) for r in ref]


# ---------------------------------------------------------------------------------------------- the route
def test_search_measure_tracker_gives_every_bit_from_the_first_whole_period():
    """mm.route_iq(): two 30 dB-Hz satellites at fractional code phases, 1000 ms.  The search on the first 220 ms, the hand-over and the
    measurement on the same buffer, then a tracker put in WAIT from the measured states replaying the buffer and going on behind it --
    against a tracker started in SYNC from the refined results.  tests/test_weak_measure_host.py asks the same of the model first."""
    from gypsum_amd.acquisition import GpsSatelliteDetector, SatelliteAcquisitionAttemptResult
    from gypsum_amd.antenna_sample_provider import SampleProviderAttributes
    from gypsum_amd.tracker import BitValue
    from gypsum_amd.weak_tracker import WeakSignalTracker
    attrs = SampleProviderAttributes(samples_per_second=mm.FS, samples_per_prn_transmission=mm.N)
    x, sats, g = mm.route_iq(), mm.route_sats(), mm.route_golden()
    head = x[:mm.ROUTE_SEARCH_MS * mm.N]
    det = GpsSatelliteDetector({})
    found = det.detect_weak_satellites_in_antenna_data([s.sat_id for s in sats], head, attrs)
    assert [f.satellite_id for f in found] == [s.sat_id for s in sats]
    for f, s, want in zip(found, sats, g["search"]):                                   # the search lands on the model's code phase, within its 10-Hz fine step
        assert f.prn_phase_shift == int(want[2]) == round(s.code_phase) and abs(f.doppler_shift - s.doppler_hz) <= 10.0, (f.doppler_shift, f.prn_phase_shift)
    measured = det.measure_weak_satellites(found, head, attrs)
    refined = det.refine_weak_satellites(found, head, attrs)
    assert [m.satellite_id for m in measured] == [s.sat_id for s in sats]
    trk = WeakSignalTracker.from_measurements(measured, attrs, 0)
    assert all(int(st["phase"]) == wm.WAIT for st in trk.bank.state())               # no SYNC
    ev_a = trk.process(head) + trk.process(x[mm.ROUTE_SEARCH_MS * mm.N:])
    sync = WeakSignalTracker(refined, attrs)
    ev_b = sync.process(x)
    # the first five period records of both, for the DLL's discriminator
    dd = []
    for results, make in ((measured, lambda: WeakSignalTracker.from_measurements(measured, attrs, 0)), (refined, lambda: WeakSignalTracker(refined, attrs))):
        t = make()
        _, per = t.bank.track_block(x, 1, 0, mm.ROUTE_MS, want_ms=False)
        dd.append([float(np.mean(np.abs(p["dd"][:5]))) for p in per])
    for c, (s, m, f) in enumerate(zip(sats, measured, found)):
        a = [e for ch, e in ev_a if ch == c]
        b = [e for ch, e in ev_b if ch == c]
        first_a, first_b = round(a[0].receiver_timestamp * 1000), round(b[0].receiver_timestamp * 1000)
        starts = [round(e.receiver_timestamp * 1000) for e in a]
        got = [1 if e.bit_value == BitValue.ONE else -1 for e in a]
        want = [mm.route_bit(s, t0) for t0 in starts]
        same = sum(int(u == v) for u, v in zip(got, want))
        err = mm.code_error(m.c0, s, mm.N)
        print(f"satellite {s.sat_id}: code phase {f.prn_phase_shift} -> {m.code_phase_samples:.3f} samples (scene {s.code_phase}), error {err:+.3f} chip, "
              f"dd_last {m.dd_last:+.4f}, C/N0 {m.cn0_dbhz:.2f} dB-Hz; first bit at {first_a} ms (from SYNC {first_b}), {same} of {len(want)} bits, "
              f"mean |dd| of five periods {dd[0][c]:.4f} (from SYNC {dd[1][c]:.4f})")
        assert m.status == 0 and m.bit_edge == (-s.bit_offset_ms) % 20 and m.correlation_strength == f.correlation_strength
        assert first_a == m.bit_edge and len(a) == (mm.ROUTE_MS - first_a) // 20 and all(v - u == 20 for u, v in zip(starts, starts[1:]))
        assert same in (0, len(want)), (s.sat_id, same, len(want))                      # every bit from the first whole period, up to the one sign
        assert first_b - first_a >= 400
        assert dd[0][c] < dd[1][c]
        # the figures the model gave on its own search result (tests/golden/weak_measure_route.npz); the device's search may hand over
        # the other 10-Hz bin, so these are bounds, not parities: the code error below the grid's, the C/N0 within the model's margin
        assert abs(err) < abs(float(g["start_error"][c])) and abs(m.cn0_dbhz - 30.0) <= 1.043 * 1.5
