"""Tracking on the recording's clock: late, gapped and per-stream start times.

Every tracking kernel wipes the carrier off at absolute receiver time t0 + n / fs, t0 from the caller's start_time array, and the
watchdog runs on differences of those times.  The rest of the suite feeds one clock shape -- round(ms N / fs, 6), gapless, within
16 s of zero -- so a precision loss in f t0 or a wrong start_time index that only shows away from t = 0 would go unnoticed.  Here:
  a. gyp_track_step, one teacher-forced millisecond at every rate, 40 s .. one GPS week, on and off the microsecond grid, every field of
     gyp_chan_out against the oracle's millisecond; three streams with three clocks in one call;
  b. the block kernels, teacher-forced from the oracle's state for six consecutive milliseconds at 40 s, one hour, one GPS week;
  c. a short closed loop at 40 s, inside the horizon the ORACLE gives (tests/test_clock_horizon.py): every integer;
  d. what the device keeps bit for bit at one hour, closed loop (block cuts, the shared exact-sums kernel, host against _dev form,
     failed speculation): late in a recording the loop amplifies a 1-ulp difference into differing integers within a dozen ms;
  e. gapped clocks near zero with a 0.3-s watchdog, closed loop against the oracle.
The bars are clock_model.bound(): float32 floor + rounding of the cycle count + the reference's own phase-rounding noise
(clock_model.reference_noise, measured per case from the oracle and its exact-phase twin).  Closed-loop parity with the oracle is
NOT defined late in a recording ("Clocks"), which is why b is teacher-forced and d needs no oracle.
"""
from __future__ import annotations

import contextlib
import time

import numpy as np
import pytest

import clock_model as cm
from gypsum_amd import _lib, synth
from gypsum_amd._lib import CHAN_IN, CHAN_INIT, TRACK_REC
from oracle import gypsum_oracle as orc
from test_gpu_track_survey import _exact, _new_tally, _tally_scene

pytestmark = pytest.mark.gpu

RATES = [1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 48]
LATE = [40.0, 3600.0, 86_400.0, cm.GPS_WEEK_S]
MIN_ARGMAX_MARGIN = 1e-5      # np.argmax's own margin in the oracle below which float32 magnitudes could order two lags differently
MIN_DISC = 1e-6               # |discriminator| / max(|E|^2, |L|^2) below which its sign -- hence int(phase) -- is not the oracle's to give
CHIPS = orc.generate_ca_codes()


# ------------------------------------------------------------------ helpers
@contextlib.contextmanager
def _switches(eng, params=None, **debug):
    """gyp_debug_set switches (and gyp_params) of a shared engine for the length of a `with`."""
    old = {k: eng.debug_get(k) for k in debug}
    old_params = eng.get_params() if params else None
    try:
        for k, v in debug.items():
            eng.debug_set(k, v)
        if params:
            eng.set_params(**params)
        yield eng
    finally:
        for k, v in old.items():
            eng.debug_set(k, v)
        if params:
            eng.set_params(**{k: old_params[k] for k in params})


def _inits(rows, streams=None):
    rec = np.zeros(len(rows), dtype=CHAN_INIT)
    for i, (sv, dop, phi, cp) in enumerate(rows):
        rec[i] = (streams[i] if streams is not None else 0, sv, dop, phi, cp, 0)
    return rec


def _fields_differing(a, b):
    """Fields of two record arrays whose bytes differ (the records' padding is not part of the result)."""
    return [f for f in a.dtype.names if a[f].tobytes() != b[f].tobytes()]


STATE_KEYS = ("doppler_hz", "carrier_phase", "code_phase", "lost")


def _state_differing(a, b, channels=None):
    """Keys of two bank.state() results whose bytes differ (all channels, or the given ones)."""
    pick = (lambda v: v) if channels is None else (lambda v: v[list(channels)])
    assert all(len(a[k]) == len(b[k]) > 0 for k in STATE_KEYS)
    return [k for k in STATE_KEYS if pick(a[k]).tobytes() != pick(b[k]).tobytes()]


def _fast(rec):
    return float(np.mean((rec["path_info"] & 3) == 1))


class _Worst:
    """Worst device error, with its bound and the reference-noise share of that bound, per key."""

    def __init__(self):
        self.w = {}

    def add(self, key, err, bound, noise):
        assert err == err and bound == bound and bound < np.inf, (key, err, bound)      # a NaN would compare False below and pass unseen
        cur = self.w.get(key)
        if cur is None or err / bound > cur[0] / cur[1]:
            self.w[key] = (err, bound, noise)

    def line(self, key):
        e, b, s = self.w[key]
        return f"{e:.2e} (bound {b:.2e}, reference noise {s:.2e})"

    def failures(self):
        return {k: v for k, v in self.w.items() if not v[0] <= v[1]}


# ------------------------------------------------------------------ a. gyp_track_step, teacher-forced, every rate
def _check_chan_out(o, r, noise, scale, f, t0, n, worst, key):
    """Every field of one gyp_chan_out against the oracle's millisecond `r`; integers asserted here, errors collected in `worst`."""
    assert r.argmax_margin >= MIN_ARGMAX_MARGIN, (key, r.argmax_margin)       # (no case is left out: the scenes were chosen for it)
    assert int(o["peak_offset"]) == r.peak_offset, (key, int(o["peak_offset"]), r.peak_offset)
    assert int(o["n_max"]) == 1, (key, int(o["n_max"]))                        # the oracle's two largest magnitudes differ: one maximum
    mag = abs(r.peak)
    b32 = lambda what: cm.bound(t0, f, "f32", noise[what])
    worst.add(key + ("peak_mag",), abs(float(o["peak_mag"]) - mag) / mag, b32("mag"), noise["mag"])
    worst.add(key + ("peak",), abs(complex(o["peak_re"], o["peak_im"]) - r.peak) / mag, b32("peak"), noise["peak"])
    pm = float(o["peak_mag"])
    strength = pm / ((float(o["sum"]) - int(o["n_max"]) * pm) / (n - int(o["n_max"])))
    worst.add(key + ("strength",), abs(strength - r.strength) / r.strength, b32("strength"), noise["strength"])
    sum_ref = mag + (n - 1) * mag / r.strength                                  # utils.py:111-116 solved for the sum of the profile
    worst.add(key + ("sum",), abs(float(o["sum"]) - sum_ref) / sum_ref, b32("strength"), noise["strength"])
    for name, want in (("early", r.early), ("late", r.late)):
        worst.add(key + (name + "32",), abs(complex(o[name + "_re"], o[name + "_im"]) - want) / scale, b32("el"), noise["el"])
        got64 = complex(o[name + "64_re"], o[name + "64_im"])
        worst.add(key + (name + "64",), abs(got64 - want) / scale, cm.bound(t0, f, "f64", noise["el"]), noise["el"])
        # beside the bound above, which grows with the reference's noise: the oracle's exact-phase twin (clock_model.exact_start) has the
        # carrier the device forms, with an argument as small as at t = 0 -- so the bar of t = 0 holds against it at every start time
        worst.add(key + (name + "64 against the exact-phase twin",), abs(got64 - getattr(noise["twin"], name)) / scale, cm.FLOAT64_FLOOR, 0.0)


@pytest.mark.parametrize("k", RATES)
def test_track_step_late_and_off_grid_at_every_rate(engine_factory, k):
    """One millisecond at T = 40 s, one hour, one day, one GPS week, on the microsecond grid and a third of a microsecond off it (f t0 is
    then not representable: so the exact fma of carrier_cycles() matters), three channels at code phases {the satellite's, 0, N - 1}:
    every field of gyp_chan_out against the oracle's millisecond, within clock_model.bound().  Then three streams at T = 0, 40 and
    3600 s in ONE call (start_time is per stream), channels interleaved across the streams: each equals its single-stream call bit
    for bit."""
    t_start = time.time()
    fs, n = 1_023_000 * k, 1023 * k
    eng = engine_factory(fs, n)
    scene = synth.random_scene(fs, 3, 3, 4100 + k, max_doppler=4800.0, with_nav_bits=False)
    iq = synth.render(scene)
    sat = scene.sats[0]
    prn = orc.prn_as_complex(CHIPS[sat.sat_id - 1], n)
    f, phi = sat.doppler_hz + 0.37, 0.8
    lags = [sat.code_phase, 0, n - 1]
    ch = np.zeros(len(lags), dtype=CHAN_IN)
    for i, s in enumerate(lags):
        ch[i] = (0, sat.sat_id, f, phi, s, 0)
    worst = _Worst()
    samples = iq[n:2 * n]
    scale = cm.el_scale(samples, n)
    for T in LATE:
        for kind in ("offset", "offgrid"):
            t0 = float(cm.clocks(n, fs, 1, kind, T, first_ms=1)[0][0])
            out, _ = eng.track_step(samples, 1, [t0], ch)
            for i, s in enumerate(lags):
                r = cm.oracle_ms(samples, prn, fs, n, f, phi, s, t0)
                noise = cm.reference_noise(samples, prn, fs, n, f, phi, s, t0, rec=r)
                _check_chan_out(out[i], r, noise, scale, f, t0, n, worst, (T, kind, s))
    for T in LATE:
        keys = [key for key in worst.w if key[0] == T]
        w32 = max((key for key in keys if not key[3].endswith("64") and not key[3].endswith("twin")), key=lambda key: worst.w[key][0] / worst.w[key][1])
        w64 = max((key for key in keys if key[3].endswith("64")), key=lambda key: worst.w[key][0] / worst.w[key][1])
        wtw = max((key for key in keys if key[3].endswith("twin")), key=lambda key: worst.w[key][0])
        print(f"[clock bounds] track_step K = {k} T = {T:g} s: float32 outputs worst {w32[3]} {worst.line(w32)}; "
              f"early64/late64 worst {worst.line(w64)}; early64/late64 against the exact-phase twin worst {worst.w[wtw][0]:.2e} (bound {worst.w[wtw][1]:.0e})")
    assert not worst.failures(), worst.failures()

    # --- three streams, three clocks, one call
    offsets = [0.0, 40.0, 3600.0]
    starts = [float(orc.chunk_times(n, n, fs)[0] + off) for off in offsets]
    streams = [iq[0:n], iq[n:2 * n], iq[2 * n:3 * n]]
    many = np.zeros(6, dtype=CHAN_IN)
    for i in range(6):
        s = scene.sats[i % len(scene.sats)]
        many[i] = (i % 3, s.sat_id, s.doppler_hz + 0.37 * i, 0.8 + 0.1 * i, lags[(i // 3 + i) % 3], 0)
    got, _ = eng.track_step(np.concatenate(streams), 3, starts, many)
    for b in range(3):
        mine = [i for i in range(6) if many[i]["stream"] == b]
        alone = many[mine].copy()
        alone["stream"] = 0
        want, _ = eng.track_step(streams[b], 1, [starts[b]], alone)
        assert not _fields_differing(got[mine], want), (k, b, _fields_differing(got[mine], want))
    print(f"[clocks a] K = {k}: {len(LATE) * 2 * len(lags)} teacher-forced channel-ms inside their bounds, 6 channels on three clocks in one "
          f"call bit-identical to single-stream calls; {time.time() - t_start:.1f} s")


# ------------------------------------------------------------------ b. block kernels, teacher-forced first millisecond
BLOCK_PATHS = [("throughput", k) for k in (1, 2, 8, 10, 20)] + [("default", k) for k in (2, 8, 16)]


@pytest.mark.parametrize("path,k", BLOCK_PATHS, ids=[f"{p}-K{k}" for p, k in BLOCK_PATHS])
def test_block_kernels_teacher_forced_late(engine_factory, path, k):
    """Six consecutive milliseconds at T = 40 s, one hour and one GPS week: a fresh 1-ms gyp_track_block from the ORACLE's state at that
    millisecond (gyp_bank_reset_dev between the calls).  The record's peak and strength within clock_model.bound(), the discriminator
    within rtol 2e-6 + the reference's own noise on it, peak offset, pseudosymbol and code phase == int(cp + disc * gain) equal.  The throughput kernel (no_spec) at one
    rate of each staging scheme, the default path where a speculative tracker exists: track_block_kernel, dll_exact_*, dll_scan_kernel
    and, where speculation is on, track_verify_kernel at late times."""
    t_start = time.time()
    fs, n = 1_023_000 * k, 1023 * k
    eng = engine_factory(fs, n)
    n_ms, first = 6, 2
    scene = synth.random_scene(fs, first + n_ms, 3, 5200 + k, max_doppler=4800.0, max_code_phase=(2046 if n > 2046 else None))
    iq = synth.render(scene)
    rng = np.random.default_rng(5200 + k)
    seeds = [(s.sat_id, float(int(round(s.doppler_hz)) + int(rng.integers(-2, 3))), float(s.carrier_phase + rng.uniform(-0.2, 0.2)), s.code_phase)
             for s in scene.sats]
    prns = [orc.prn_as_complex(CHIPS[sv - 1], n) for sv, _, _, _ in seeds]
    worst = _Worst()
    paths_seen = set()
    with _switches(eng, no_spec=1 if path == "throughput" else 0):
        bank = eng.create_bank(_inits(seeds))
        dev = eng.alloc(len(seeds) * CHAN_INIT.itemsize)
        try:
            for T in (40.0, 3600.0, cm.GPS_WEEK_S):
                start, end = cm.clocks(n, fs, n_ms, "offset", T, first_ms=first)
                # the oracle's own closed loop gives the states (chaotic or not late in a recording: each millisecond is compared from ITS state)
                loops = [cm.oracle_rows(iq, prns[i], fs, n, seeds[i][1:], start, end, first)[0] for i in range(len(seeds))]
                assert all(len(rows) == n_ms for rows in loops)
                for j in range(n_ms):
                    state = [(seeds[i][0], loops[i][j].doppler_used, loops[i][j].carrier_phase_used, loops[i][j].code_phase_used) for i in range(len(seeds))]
                    dev.upload(_inits(state))
                    bank.reset_dev(dev.ptr.value)
                    eng.sync()
                    samples = iq[(first + j) * n:(first + j + 1) * n]
                    rec = bank.track_block(samples, 1, 1, [start[j]])
                    for i, (sv, f, phi, cp) in enumerate(state):
                        g = rec[i, 0]
                        key = (T, j, i)
                        r = cm.oracle_ms(samples, prns[i], fs, n, f, phi, cp, float(start[j]))
                        noise = cm.reference_noise(samples, prns[i], fs, n, f, phi, cp, float(start[j]), rec=r)
                        e2, l2 = abs(r.early) ** 2, abs(r.late) ** 2
                        assert r.argmax_margin >= MIN_ARGMAX_MARGIN, (key, r.argmax_margin)
                        assert abs(r.discriminator) >= MIN_DISC * max(e2, l2), (key, r.discriminator)
                        paths_seen.add(int(g["path_info"]) & 3)
                        assert int(g["status"]) == 0 and bool(g["nudged"]) == bool(r.nudged), key
                        assert int(g["peak_offset"]) == r.peak_offset, (key, int(g["peak_offset"]), r.peak_offset)
                        assert int(g["pseudosymbol"]) == r.pseudosymbol, key
                        assert int(g["code_phase"]) == int(cp + r.discriminator * orc.DLL_GAIN) == r.code_phase_after, (key, int(g["code_phase"]))
                        # rtol 2e-6, atol 1e-6 as test_forced_repairs_leave_records_and_state_exact, plus -- the structure of every bound here -- the
                        # reference's own noise on this very number (oracle against exact-phase twin; 3e-6 .. 7e-6 relative at one GPS week)
                        tol = 2e-6 * abs(r.discriminator) + 1e-6 + noise["disc"]
                        worst.add((T, "discriminator"), abs(float(g["discriminator"]) - r.discriminator), tol, noise["disc"])
                        mag = abs(r.peak)
                        worst.add((T, "peak"), abs(complex(g["peak_re"], g["peak_im"]) - r.peak) / mag, cm.bound(start[j], f, "f32", noise["peak"]), noise["peak"])
                        worst.add((T, "strength"), abs(float(g["strength"]) - r.strength) / r.strength,
                                  cm.bound(start[j], f, "f32", noise["strength"]), noise["strength"])
        finally:
            dev.free()
            bank.close()
    for T in (40.0, 3600.0, cm.GPS_WEEK_S):
        print(f"[clock bounds] track_block {path} K = {k} T = {T:g} s: peak worst {worst.line((T, 'peak'))}; strength worst {worst.line((T, 'strength'))}; "
              f"discriminator (absolute) worst {worst.line((T, 'discriminator'))}")
    print(f"[clocks b] {path} K = {k}: {3 * n_ms * len(seeds)} teacher-forced channel-ms, path_info & 3 seen {sorted(paths_seen)}; {time.time() - t_start:.1f} s")
    assert not worst.failures(), worst.failures()


# ------------------------------------------------------------------ c. a short closed loop inside the reference's horizon
@pytest.mark.parametrize("k", [2, 8])
def test_short_closed_loop_at_40_s_inside_the_oracles_horizon(engine_factory, k):
    """min(8, horizon(40) - 2) milliseconds from a fresh bank in ONE block at T = 40 s, both kernels: every integer of every planned
    channel-millisecond equals the oracle's (no excuse mechanism).  The horizon is clock_model.horizon(): the oracle against its own
    float32-perturbed twin on the same scenes, no device in it.  Reaches the milliseconds after a block's first at a late time: the
    speculative kernel's t0_next, the Costas candidates, the window maxima."""
    t_start = time.time()
    fs, n = 1_023_000 * k, 1023 * k
    eng = engine_factory(fs, n)
    T = 40.0
    hz = cm.horizon(fs, T)
    n_ms = min(8, hz - 2)
    assert n_ms >= 4, hz                                     # (oracle only: the scenes leave a loop worth running)
    first = cm.HORIZON_FIRST_MS
    start, end = cm.clocks(n, fs, n_ms, "offset", T, first_ms=first)
    iqs, seeds, streams = [], [], []
    for b, regime in enumerate(("lock", "pull-in")):
        iq, inits = cm.horizon_scene(fs, first + cm.HORIZON_N_MS, regime)
        iqs.append(iq[first * n:(first + n_ms) * n])
        seeds += inits
        streams += [b] * len(inits)
    want = [cm.oracle_rows(iqs[streams[i]], orc.prn_as_complex(CHIPS[seeds[i][0] - 1], n), fs, n, seeds[i][1:], start, end, 0)[0] for i in range(len(seeds))]
    assert all(len(w) == n_ms for w in want)
    for label, no_spec in (("throughput", 1), ("default", 0)):
        with _switches(eng, no_spec=no_spec):
            bank = eng.create_bank(_inits(seeds, streams))
            rec = bank.track_block(np.concatenate(iqs), 2, n_ms, start)
            bank.close()
        for i, rows in enumerate(want):
            for name, attr in (("code_phase", "code_phase_after"), ("peak_offset", "peak_offset"), ("pseudosymbol", "pseudosymbol"),
                               ("locked", "locked"), ("nudged", "nudged")):
                assert [int(v) for v in rec[i][name]] == [int(getattr(r, attr)) for r in rows], (label, k, i, name)
            assert not rec[i]["status"].any(), (label, i)
        print(f"[clocks c] {label} K = {k}: {len(seeds)} channels x {n_ms} ms at T = 40 s equal to the oracle (oracle's horizon {hz} ms), "
              f"fast-path share {_fast(rec):.2f}")
    print(f"[clocks c] K = {k}: {time.time() - t_start:.1f} s")


# ------------------------------------------------------------------ d. bit-for-bit invariants at one hour
LATE_MS = 120
CUTS = (1, 37, 64, 3, 15)


def _late_scene(fs, n, with_absent):
    scene = synth.random_scene(fs, 9 + LATE_MS, 4, 9911, max_code_phase=(2046 if n > 2046 else None))
    iq = synth.render(scene)[9 * n:]
    rows = [(s.sat_id, float(round(s.doppler_hz)), s.carrier_phase, s.code_phase) for s in scene.sats]
    if with_absent:          # noise-only channels: with kappa = 0 their verification must fail (test_failed_speculation_is_recovered_bit_for_bit)
        present = {s.sat_id for s in scene.sats}
        absent = [sv for sv in range(1, 33) if sv not in present][:3]
        rows += [(sv, 1000.0 * (j - 1), 0.5, 100 + 700 * j) for j, sv in enumerate(absent)]
    return iq, _inits(rows), len(scene.sats)


def _run_blocks(eng, iq, inits, n, t0, cuts):
    bank = eng.create_bank(inits)
    try:
        parts, at = [], 0
        for cut in cuts:
            parts.append(bank.track_block(iq[at * n:(at + cut) * n], 1, cut, t0[at:at + cut]))
            at += cut
        bad = np.zeros(len(inits), dtype=np.int32)
        eng._check(eng.lib.gyp_debug_spec_read(bank.handle, None, 0, _lib.ptr(bad)))
        return np.concatenate(parts, axis=1), bank.state(), bad
    finally:
        bank.close()


@pytest.mark.parametrize("k", [8, 2])
def test_block_cuts_change_nothing_at_one_hour(engine_factory, k):
    """T = 3600 s, 120 ms closed loop: one block == the ragged blocks (1, 37, 64, 3, 15) on both kernels, every record field and the
    final state as bytes.  Needs no oracle: at one hour the loop turns any path-dependent rounding into differing integers."""
    t_start = time.time()
    fs, n = 1_023_000 * k, 1023 * k
    eng = engine_factory(fs, n)
    iq, inits, _ = _late_scene(fs, n, False)
    t0 = cm.clocks(n, fs, LATE_MS, "offset", 3600.0, first_ms=9)[0]
    for label, no_spec in (("throughput", 1), ("default", 0)):
        with _switches(eng, no_spec=no_spec):
            whole, st_w, _ = _run_blocks(eng, iq, inits, n, t0, (LATE_MS,))
            cut, st_c, _ = _run_blocks(eng, iq, inits, n, t0, CUTS)
        fast = _fast(whole)
        diff = _fields_differing(cut, whole)          # (path_info included: the same windows and confidences, however the block is cut)
        print(f"[clocks d] cuts, {label} K = {k}: fast-path share {fast:.2f} (whole) {_fast(cut):.2f} (cut), differing fields {diff}")
        assert (fast > 0.5) == (label == "default"), (label, fast)          # it really was the path it is named after
        assert not diff, (label, k, diff)
        assert not _state_differing(st_w, st_c), (label, k, _state_differing(st_w, st_c))
    print(f"[clocks d] cuts K = {k}: {time.time() - t_start:.1f} s")


def test_exact_paths_and_call_forms_agree_at_one_hour(engine_factory):
    """T = 3600 s, 120 ms closed loop at 8 samples per chip: the shared exact-sums kernel against the per-channel one
    ("no_exact_shared" 0 / 1) on the throughput path, and the host form gyp_track_block against gyp_track_block_dev on both kernels:
    records and final state as bytes."""
    t_start = time.time()
    fs, n = 8_184_000, 8184
    eng = engine_factory(fs, n)
    iq, inits, _ = _late_scene(fs, n, False)
    t0 = cm.clocks(n, fs, LATE_MS, "offset", 3600.0, first_ms=9)[0]
    with _switches(eng, no_spec=1, no_exact_shared=0):
        shared, st_s, _ = _run_blocks(eng, iq, inits, n, t0, (LATE_MS,))
        assert eng.debug_get("last_exact_path") == 2
    with _switches(eng, no_spec=1, no_exact_shared=1):
        wave, st_v, _ = _run_blocks(eng, iq, inits, n, t0, (LATE_MS,))
        assert eng.debug_get("last_exact_path") == 1
    assert not _fields_differing(wave, shared), _fields_differing(wave, shared)
    assert not _state_differing(st_s, st_v), _state_differing(st_s, st_v)
    for label, no_spec in (("throughput", 1), ("default", 0)):
        with _switches(eng, no_spec=no_spec):
            host, st_h, _ = _run_blocks(eng, iq, inits, n, t0, (LATE_MS,))
            d_iq = eng.alloc(iq.nbytes).upload(iq)
            d_t0 = eng.alloc(t0.nbytes).upload(t0)
            d_rec = eng.alloc(len(inits) * LATE_MS * TRACK_REC.itemsize)
            bank = eng.create_bank(inits)
            try:
                bank.track_block_dev(d_iq.ptr.value, LATE_MS * n, LATE_MS, d_t0.ptr.value, d_rec.ptr.value)
                eng.sync()
                dev = d_rec.download(TRACK_REC, len(inits) * LATE_MS).reshape(len(inits), LATE_MS)
                st_d = bank.state()
            finally:
                bank.close()
                for d in (d_iq, d_t0, d_rec):
                    d.free()
        assert (_fast(host) > 0.5) == (label == "default"), (label, _fast(host))
        assert not _fields_differing(dev, host), (label, _fields_differing(dev, host))
        assert not _state_differing(st_d, st_h), (label, _state_differing(st_d, st_h))
    print(f"[clocks d] exact-sums kernels and call forms agree at T = 3600 s; {time.time() - t_start:.1f} s")


def test_failed_speculation_is_recovered_bit_for_bit_at_one_hour(engine_factory):
    """test_failed_speculation_is_recovered_bit_for_bit's assertion on the late clock: kappa = 0 trusts every interior window maximum, the
    noise-only channels fail verification, and every channel that did is the transform kernel's, bit for bit -- at T = 3600 s."""
    t_start = time.time()
    fs, n = 8_184_000, 8184
    eng = engine_factory(fs, n)
    iq, inits, n_present = _late_scene(fs, n, True)
    t0 = cm.clocks(n, fs, LATE_MS, "offset", 3600.0, first_ms=9)[0]
    with _switches(eng, no_spec=1):
        rec_t, st_t, _ = _run_blocks(eng, iq, inits, n, t0, (LATE_MS,))
    with _switches(eng, params={"spec_confidence_kappa": 0.0}, no_spec=0):
        rec_s, st_s, bad = _run_blocks(eng, iq, inits, n, t0, (LATE_MS,))
    print(f"[clocks d] kappa = 0 at T = 3600 s: failed verification {bad.tolist()}, fast-path share per channel "
          f"{[round(_fast(rec_s[i]), 2) for i in range(len(inits))]}")
    assert bad[n_present:].all(), bad
    for i in np.nonzero(bad)[0]:
        assert rec_s[i].tobytes() == rec_t[i].tobytes(), (i, _fields_differing(rec_s[i], rec_t[i]))
        assert np.all((rec_s[i]["path_info"] & 3) == 0)
    assert not _state_differing(st_s, st_t, np.nonzero(bad)[0]), _state_differing(st_s, st_t, np.nonzero(bad)[0])
    print(f"[clocks d] failed speculation: {time.time() - t_start:.1f} s")


# ------------------------------------------------------------------ e. irregular clocks near zero, closed loop against the oracle
def _rows_for_tally(rows, n_ms):
    """clock_model.oracle_rows -> the per-ms rows of survey_worker.run_scene (what _tally_scene reads)."""
    out = np.zeros((n_ms, 12), dtype=np.float64)
    out[:, 11] = np.nan
    out[len(rows):, 5] = 1.0
    for j, r in enumerate(rows):
        out[j, :11] = (r.pseudosymbol, r.code_phase_after, r.peak_offset, float(r.locked), r.doppler_after, 0.0, float(r.nudged),
                       r.lock_margin, abs(r.peak.real) / max(abs(r.peak), 1e-300), r.argmax_margin, abs(r.peak))
    return out


# gyp_params the watchdog reads -> the oracle's constants.  "looks": the period alone (the looks the jumps trigger or suppress change the
# device's last-look time, which later looks depend on); "nudges": thresholds at which a look also nudges, so each look shows in the records
WATCHDOGS = {"looks": {"watchdog_period_s": 0.3},
             "nudges": {"watchdog_period_s": 0.3, "watchdog_drop_below": 0.02, "watchdog_nudge_below": 0.995, "watchdog_nudge_hz": 3.0}}
ORACLE_NAME = {"watchdog_period_s": "WATCHDOG_PERIOD_S", "watchdog_drop_below": "WATCHDOG_DROP_BELOW",
               "watchdog_nudge_below": "WATCHDOG_NUDGE_BELOW", "watchdog_nudge_hz": "WATCHDOG_NUDGE_HZ"}


def _gapped_against_the_oracle(eng, fs, n, seed, n_ms, jumps, label, no_spec, watchdog):
    first = 9
    params = WATCHDOGS[watchdog]
    scene = synth.lock_regime_scene(fs, first + n_ms, seed)
    iq = synth.render(scene)
    rng = np.random.default_rng(seed ^ 0x5EED)
    seeds = [(s.sat_id, float(int(round(s.doppler_hz)) + int(rng.integers(-2, 3))),
              float(np.angle(np.exp(1j * (s.carrier_phase + rng.uniform(-0.2, 0.2))))), s.code_phase) for s in scene.sats]
    start, end = cm.clocks(n, fs, n_ms, "gapped", jumps, first_ms=first)
    assert start.max() < 10.0
    old = {name: getattr(orc, ORACLE_NAME[name]) for name in params}
    for name, v in params.items():
        setattr(orc, ORACLE_NAME[name], v)
    try:
        traj = [_rows_for_tally(cm.oracle_rows(iq, orc.prn_as_complex(CHIPS[sv - 1], n), fs, n, (dop, phi, cp), start, end, first, margins=True)[0], n_ms)
                for sv, dop, phi, cp in seeds]
    finally:
        for name, v in old.items():
            setattr(orc, ORACLE_NAME[name], v)
    with _switches(eng, params=params, no_spec=no_spec):
        bank = eng.create_bank(_inits(seeds))
        rec = bank.track_block(iq[first * n:], 1, n_ms, start)
        bank.close()
    tally = _new_tally(None)
    _tally_scene(rec, seed, traj, tally, label, None)
    for i, rows in enumerate(traj):
        alive = int((rows[:, 5] == 0).sum())
        assert not rec[i, :alive]["status"].any(), (label, i)
        assert np.array_equal(rec[i, :alive]["nudged"] != 0, rows[:alive, 6] != 0), (label, i)
        if alive < n_ms:
            assert int(rec[i, alive]["status"]) == 1 and np.all(rec[i, alive + 1:]["status"] == 2), (label, i, alive)
    print(f"[clocks e] {label}: {tally['n']} channel-ms on a clock with jumps {jumps}, {tally['nudges']} watchdog nudges, {tally['lost']} channels "
          f"dropped by the watchdog, fast-path ms {tally['fast']}, worst prompt |.| difference {tally['mag']:.1e}")
    _exact(tally)
    assert tally["nudge_bad"] == 0
    return tally


GAP_JUMPS = [(100, 2.5), (250, -1.0), (400, 0.4003337)]


@pytest.mark.parametrize("watchdog", list(WATCHDOGS))
@pytest.mark.parametrize("no_spec", [1, 0], ids=["throughput", "default"])
def test_gapped_clock_with_a_short_watchdog_against_the_oracle(engine_factory, no_spec, watchdog):
    """2.046 Msps, lock-regime scene, 700 ms, all times below 10 s, watchdog_period_s = 0.3 on both sides (alone, and
    with thresholds at which a look also nudges): the clock jumps by +2.5 s at
    block millisecond 100 (a look in mid-block), by -1.0 s at 250 (the first millisecond of the throughput kernel's second 250-ms launch:
    looks are suppressed for 1.3 s) and by +0.4003337 s (no whole number of milliseconds, off the microsecond grid) at 400.  The bars of
    _exact() in tests/test_gpu_track_survey.py, plus `nudged` and `status` equal."""
    t_start = time.time()
    fs, n = 2_046_000, 2046
    t = _gapped_against_the_oracle(engine_factory(fs, n), fs, n, 11, 700, GAP_JUMPS, f"gapped clock K = 2 {'throughput' if no_spec else 'default'}, {watchdog}", no_spec, watchdog)
    assert (t["fast"] > 0) == (not no_spec)
    if watchdog == "nudges":
        assert t["nudges"] > 0                       # (oracle only: the looks are visible in the records)
    print(f"[clocks e] K = 2: {time.time() - t_start:.1f} s")


@pytest.mark.parametrize("watchdog", list(WATCHDOGS))
def test_gapped_clock_across_verify_sub_blocks_against_the_oracle(engine_factory, watchdog):
    """8.184 Msps, 300 ms on the default (speculative) path cut into 100-ms verify sub-blocks ("spec_sub_ms"): jumps at block millisecond
    50 and at the first millisecond of the second and third sub-block (gyp_debug_spec_layout_for)."""
    t_start = time.time()
    fs, n = 8_184_000, 8184
    eng = engine_factory(fs, n)
    starts = np.zeros(33, dtype=np.int32)
    n_sub = eng.lib.gyp_debug_spec_layout_for(300, 100, _lib.ptr(starts))
    assert n_sub >= 3, (n_sub, starts[:n_sub + 1])
    jumps = [(50, 2.5), (int(starts[1]), -1.0), (int(starts[2]), 0.4003337)]
    with _switches(eng, spec_sub_ms=100):
        t = _gapped_against_the_oracle(eng, fs, n, 11, 300, jumps, f"gapped clock K = 8 default, {watchdog}", 0, watchdog)
    assert t["fast"] > 0.5 * t["n"]
    if watchdog == "nudges":
        assert t["nudges"] > 0
    print(f"[clocks e] K = 8, sub-blocks at {starts[:n_sub + 1].tolist()}: {time.time() - t_start:.1f} s")
