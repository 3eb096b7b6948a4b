"""The weak bank on the device (include/gypsum_hip.h, "weak-signal tracking") against the float64 model of tests/weak_track_model.py:
teacher-forced periods at every rate, the closed loop on the scene of tests/weak_track_scene.py against the recorded model run,
bitwise invariance under splitting the recording into calls and under the bank's other channels, the refusals, and the path from
the weak-signal search through WeakSignalTracker to navigation bits.

Measured on one MI355X (profiles/weak_track_kernels.txt): teacher-forced per-millisecond sums within 8.2e-6 ||x_ms||_2 of the model
at 49.104 Msps, 1.5e-6 at 1.023 Msps (bar 1e-4; the float32 half-ulp of a noise-free prompt is of that size); closed loop, largest
|device - model| over all periods and channels as a share of the model's rms tracking jitter: f 2.4e-7, u0 2.5e-7, c0 5.3e-7 (bar 1e-3).
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import weak_track_model as wm
import weak_track_scene as ws
from gypsum_amd import _lib, _records
from gypsum_amd.engine import GypsumEngine
from gypsum_amd.gps_ca_prn_codes import generate_ca_code_table

pytestmark = pytest.mark.gpu

BAD_ARG = _lib.GYP_E_BAD_ARG
MULTIPLES = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 48)          # gyp_set_stream_format's rate list


def inits_of(rows) -> np.ndarray:
    """CHAN_INIT records from (stream, init dict of weak_track_scene.inits()) pairs."""
    out = np.zeros(len(rows), dtype=_lib.CHAN_INIT)
    for i, (stream, d) in enumerate(rows):
        out[i] = (stream, d["sat_id"], d["doppler_hz"], d["carrier_phase"], d["code_phase"], 0)
    return out


def cplx(ms: np.ndarray, name: str) -> np.ndarray:
    return ms[name + "_re"].astype(np.float64) + 1j * ms[name + "_im"].astype(np.float64)


# ---------------------------------------------------------------------------------------------- teacher-forced
def forced_states(n: int):
    """(f, u0, c0) of the forced channels: the code phase 3 samples before the 1023-chip wrap with Doppler +10 kHz and u0 = 0.999;
    Doppler -10 kHz from the middle of the code; a state a quarter sample off the first one's code."""
    k = n // 1023
    per_sample = wm.ONE // k
    near_wrap = wm.CODE_MOD - 3 * per_sample + per_sample // 2
    return [(10000.0, 0.999, near_wrap), (-10000.0, 0.25, 511 * wm.ONE + 12345), (10000.0 + 37.0, 0.5, (near_wrap + per_sample // 4) % wm.CODE_MOD),
            (-4000.25, 0.0, 0)]


@pytest.mark.parametrize("mult", MULTIPLES)
def test_teacher_forced_period_matches_the_model(engine_factory, mult):
    n, fs = 1023 * mult, 1_023_000 * mult
    eng = engine_factory(fs, n)
    sat, a, sigma = 11, 0.01, 0.05
    chips = generate_ca_code_table()[sat - 1].astype(np.float64) * 2 - 1
    spacing = wm.ONE // mult                       # one sample (half a chip at 2.046 Msps: the default)
    states = forced_states(n)
    f0, u0, c0 = states[0]
    # stream 0: the noise-free signal that channel 0's replica matches sample for sample; stream 1: the same under noise
    k = np.arange(20 * n, dtype=np.int64)
    du = np.float64(f0) / np.float64(fs)
    u = np.float64(u0) + du * k.astype(np.float64)
    clean = a * chips[wm.chip_index(c0, 0, k, wm.code_rate(f0, n))] * np.exp(2j * np.pi * (u - np.rint(u)))
    rng = np.random.default_rng(mult)
    noisy = clean + sigma * (rng.standard_normal(20 * n) + 1j * rng.standard_normal(20 * n))
    x = np.stack([clean, noisy]).astype(np.complex64)
    prm = _records.WeakParams(spacing=spacing)
    inits = np.zeros(2 * len(states), dtype=_lib.CHAN_INIT)
    for i in range(len(inits)):
        inits[i] = (i // len(states), sat, 0.0, 0.0, 0, 0)
    bank = eng.create_weak_bank(inits, prm, 0)
    for i in range(len(inits)):
        f, uu, cc = states[i % len(states)]
        bank.set_state(i, f, f, uu, cc, 0)
    ms, per = bank.track_block(x, 2, 0, 20)
    worst = 0.0
    for i in range(len(inits)):
        f, uu, cc = states[i % len(states)]
        xs = x[i // len(states)]
        r = wm.code_rate(f, n)
        assert len(per[i]) == 1
        p = per[i][0]
        assert (float(p["f"]), float(p["u0"]), int(p["c0"]), int(p["first_ms"]), int(p["status"])) == (f, uu, cc, 0, 0)
        tot = 0j
        for j in range(20):
            xm = xs[j * n:(j + 1) * n]
            want = wm.ms_sums(xm, chips, fs, uu, f, j * n, cc, r, spacing)
            bar = 1e-4 * float(np.linalg.norm(xm.astype(np.complex128)))
            rec = ms[i, j]
            assert (int(rec["phase"]), int(rec["pos"]), int(rec["status"])) == (wm.TRACK, j, 0)
            for name, w in zip(("minus", "prompt", "plus"), want):
                err = abs(complex(cplx(rec, name)) - w)
                worst = max(worst, err / (bar / 1e-4))
                assert err <= bar, (mult, i, j, name, err, bar)
            if i == 0:       # the matched, noise-free channel: every chip index right means prompt = a N (one wrong chip costs 2 a >> the bar)
                assert abs(complex(cplx(rec, "prompt")) - a * n) <= bar, (mult, j)
            tot += complex(np.complex64(want[1]))
        assert abs(complex(p["i"], p["q"]) - tot) <= 20 * 1e-4 * float(np.linalg.norm(xs[:n].astype(np.complex128)))
        assert int(p["bit"]) == (1 if p["i"] >= 0 else -1)
    print(f"{fs} Hz: largest |device - model| / ||x_ms||_2 = {worst:.3g}")
    st = bank.state()
    assert all(int(s["phase"]) == wm.TRACK and int(s["n_periods"]) == 1 and int(s["pos"]) == 0 for s in st) and bank.cursor == 20
    bank.close()


# ---------------------------------------------------------------------------------------------- closed loop on the scene
def scene_bank(eng, first_ms=0):
    return eng.create_weak_bank(inits_of([(0, d) for d in ws.inits()]), None, first_ms)


def run_split(eng, sizes):
    """The scene through a fresh bank in calls of the given sizes (the last one repeated to the end): (ms records, period lists)."""
    bank = scene_bank(eng)
    x = ws.iq()
    at, i, ms_parts, per = 0, 0, [], [[] for _ in range(bank.n_chan)]
    while at < ws.N_MS:
        step = min(sizes[min(i, len(sizes) - 1)], ws.N_MS - at)
        ms, pp = bank.track_block(x[at * ws.N:(at + step) * ws.N], 1, at, step)
        ms_parts.append(ms)
        for c in range(bank.n_chan):
            per[c].append(pp[c])
        at, i = at + step, i + 1
    state = bank.state()
    bank.close()
    return np.concatenate(ms_parts, axis=1), [np.concatenate(p) for p in per], state


@pytest.fixture(scope="module")
def one_call(engine_factory):
    return run_split(engine_factory(ws.FS, ws.N), [ws.N_MS])


def test_closed_loop_matches_the_recorded_model_run(one_call):
    ms, per, state = one_call
    g = ws.golden()
    worst = {"f": 0.0, "u0": 0.0, "c0": 0.0}
    for c, sv in enumerate(ws.CHANNEL_SATS):
        k = int(g["n_periods"][c])
        assert len(per[c]) == k, sv                                                   # the period count
        assert int(state[c]["edge"]) == int(g["edge"][c]), sv                         # the bit edge
        assert np.array_equal(per[c]["first_ms"], g["first_ms"][c, :k]), sv
        assert np.array_equal(per[c]["bit"], g["bit"][c, :k].astype(np.int32)), sv    # every bit
        assert np.array_equal(per[c]["status"], g["status"][c, :k].astype(np.int32)), sv
        lost = int(g["lost_at_ms"][c])
        dev_lost = np.flatnonzero(ms[c]["status"] == 2)
        assert (int(dev_lost[0]) if dev_lost.size else -1) == lost, sv                # the millisecond at which a channel is lost
        if lost >= 0:
            assert np.all(ms[c]["status"][lost:] == 2) and not ms[c][lost:].tobytes().replace(b"\x02", b"\0").strip(b"\0")
        du = np.abs((per[c]["u0"] - g["u0"][c, :k] + 0.5) % 1.0 - 0.5)
        dc = np.abs((per[c]["c0"] - g["c0"][c, :k] + wm.CODE_MOD // 2) % wm.CODE_MOD - wm.CODE_MOD // 2).astype(np.float64)
        df = np.abs(per[c]["f"] - g["f"][c, :k])
        for name, d in (("f", df), ("u0", du), ("c0", dc)):
            share = float(d.max()) / float(g["jitter_" + name][c])
            worst[name] = max(worst[name], share)
            print(f"satellite {sv}: largest |device - model| of {name} = {d.max():.3g} = {share:.3g} of the model's rms jitter {g['jitter_' + name][c]:.3g}")
            assert share <= 1e-3, (sv, name, share)
    print("largest shares:", worst)
    absent = len(ws.CHANNEL_SATS) - 1
    assert int(state[absent]["status"]) == 2 and all(int(s["status"]) == 0 for s in state[:absent])
    assert all(float(s["mu_mean"]) >= 4.0 for s in state[:absent])


SPLITS = {"ragged": [1, 19, 20, 21, 399, 1, 2, ws.N_MS], "all-20s": [20], "all-7s": [7]}


@pytest.mark.parametrize("name", sorted(SPLITS))
def test_records_do_not_depend_on_how_the_recording_is_split(engine_factory, one_call, name):
    ms, per, state = run_split(engine_factory(ws.FS, ws.N), SPLITS[name])
    assert ms.tobytes() == one_call[0].tobytes()
    for c in range(len(per)):
        assert per[c].tobytes() == one_call[1][c].tobytes(), c
    assert state.tobytes() == one_call[2].tobytes()


def test_records_do_not_depend_on_the_banks_other_channels(engine_factory, one_call):
    """Banks of 1, 5 and 7 channels over two streams a stride larger than n_ms N apart, three calls of 600 ms.  In the largest bank
    a mate is dropped and a live one restarted at the first boundary, one is lost by itself inside the second call (the absent
    satellite, at the scene's millisecond), and at the second boundary the dropped slot and the lost slot -- both status 2 by then --
    are revived with set_channel: they come back in SYNC at the cursor with status 0 and track."""
    eng = engine_factory(ws.FS, ws.N)
    n_ms, part, lag = 1800, 600, 40
    x = ws.iq()
    stride = n_ms * ws.N + 77
    both = np.zeros(2 * stride, dtype=np.complex64)
    both[:n_ms * ws.N] = x[:n_ms * ws.N]
    both[stride:stride + n_ms * ws.N] = x[lag * ws.N:(lag + n_ms) * ws.N]
    d = {i["sat_id"]: i for i in ws.inits()}
    tr = ws.truth()

    def init_at(stream, sv, ms):
        """A start for satellite sv at millisecond ms of the scene: 4 Hz off, the code phase where its code Doppler has carried it."""
        cp = round(tr[sv].code_phase - ms * ws.N * tr[sv].doppler_hz / wm.L1_HZ) % ws.N
        return inits_of([(stream, dict(sat_id=sv, doppler_hz=tr[sv].doppler_hz + ws.INIT_OFFSET_HZ, carrier_phase=0.7, code_phase=cp))])[0]

    layouts = {1: [(0, d[7])],
               5: [(0, d[7]), (0, d[19]), (1, d[3]), (0, d[22]), (1, d[26])],
               7: [(1, d[3]), (1, d[15]), (0, d[22]), (0, d[7]), (1, d[26]), (0, d[12]), (0, d[19])]}
    d_iq = eng.alloc(both.nbytes).upload(both)
    got, states = {}, {}
    try:
        for size, rows in layouts.items():
            bank = eng.create_weak_bank(inits_of(rows), None, 0)
            mp = bank.max_periods(part)
            d_ms, d_per, d_cnt = eng.alloc(size * part * _lib.WEAK_MS_REC.itemsize), eng.alloc(size * mp * _lib.WEAK_PERIOD_REC.itemsize), eng.alloc(size * 4)
            ms_parts, per_parts = [], [[] for _ in rows]
            for call in range(3):
                if size == 7 and call == 1:
                    bank.drop_channel(1)                              # a mate dropped mid-run ...
                    bank.set_channel(5, init_at(0, 12, part))         # ... and a live one restarted in SYNC at the cursor
                if size == 7 and call == 2:
                    states["before"] = bank.state()
                    bank.set_channel(1, init_at(1, 15, 2 * part + lag))   # the dropped slot revived on stream 1 (40 ms ahead of stream 0) ...
                    bank.set_channel(2, init_at(0, 3, 2 * part))          # ... and the slot that was lost inside the second call, on stream 0
                    states["after"] = bank.state()
                bank.track_block_dev(d_iq.ptr.value + 8 * call * part * ws.N, stride, call * part, part, d_ms.ptr.value, d_per.ptr.value, d_cnt.ptr.value)
                eng.sync()
                ms_parts.append(d_ms.download(_lib.WEAK_MS_REC, size * part).reshape(size, part))
                cnt = d_cnt.download(np.int32, size)
                pr = d_per.download(_lib.WEAK_PERIOD_REC, size * mp).reshape(size, mp)
                for c in range(size):
                    per_parts[c].append(pr[c, :cnt[c]])
            if size == 7:
                states["end"] = bank.state()
            got[size] = {(s, r["sat_id"]): (np.concatenate([m[c] for m in ms_parts]), np.concatenate(per_parts[c])) for c, (s, r) in enumerate(rows)}
            for b in (d_ms, d_per, d_cnt):
                b.free()
            bank.close()
    finally:
        d_iq.free()
    # the other channels' records are the same bits in every bank, whatever happened to their mates
    for key in ((0, 7),):
        for size in (5, 7):
            assert got[size][key][0].tobytes() == got[1][key][0].tobytes() and got[size][key][1].tobytes() == got[1][key][1].tobytes(), (size, key)
    for key in ((0, 19), (1, 3), (1, 26)):
        assert got[7][key][0].tobytes() == got[5][key][0].tobytes() and got[7][key][1].tobytes() == got[5][key][1].tobytes(), key
    # the single channel is the scene's first 1800 ms: the same bits as the seven-channel scene bank gave
    assert got[1][(0, 7)][0].tobytes() == one_call[0][0, :n_ms].tobytes()
    # lost: the absent satellite, in both banks at the scene's millisecond, status-2 records from then on
    lost = int(ws.golden()["lost_at_ms"][-1])
    assert part < lost < 2 * part
    for size in (5, 7):
        st = got[size][(0, 22)][0]["status"]
        assert st[lost - 1] == 0 and np.all(st[lost:2 * part] == 2), size
    assert np.all(got[5][(0, 22)][0]["status"][lost:] == 2)
    # dropped at the first boundary: status 2 through the second call; restarted live at the first boundary: SYNC again, then TRACK
    ms15, ms12, ms22 = got[7][(1, 15)][0], got[7][(0, 12)][0], got[7][(0, 22)][0]
    assert np.all(ms15["status"][:part] == 0) and np.all(ms15["status"][part:2 * part] == 2)
    assert np.all(ms12["status"] == 0) and np.all(ms12["phase"][part:part + 400] == wm.SYNC) and ms12["phase"][2 * part - 1] == wm.TRACK
    # revived at the second boundary: both slots were status 2, come back in SYNC at the cursor with status 0 and no periods, and track
    assert int(states["before"][1]["status"]) == 2 and int(states["before"][2]["status"]) == 2
    for slot, key, edge in ((1, (1, 15), ws.true_edge(tr[15])), (2, (0, 22), ws.true_edge(tr[3]))):
        a = states["after"][slot]
        assert (int(a["status"]), int(a["phase"]), int(a["edge"]), int(a["n_periods"]), int(a["pos"])) == (0, wm.SYNC, -1, 0, 0), slot
        ms, per = got[7][key]
        assert np.all(ms["status"][2 * part:] == 0) and np.all(ms["phase"][2 * part:2 * part + 400] == wm.SYNC) and ms["phase"][-1] == wm.TRACK, slot
        late = per[per["first_ms"] >= 2 * part]
        assert len(late) == 9 and late["first_ms"][0] == min(m for m in range(2 * part + 400, 2 * part + 420) if m % 20 == edge), slot
        assert np.all(np.diff(late["first_ms"]) == 20) and np.all(late["status"] == 0)
        # noise alone gives mu = 1 +- 0.2 per period; the model's periods from these starts have mu 9.4 and above
        assert float(late["mu"].min()) >= 4.0, (slot, late["mu"])
        e = states["end"][slot]
        assert (int(e["status"]), int(e["phase"]), int(e["edge"]), int(e["n_periods"])) == (0, wm.TRACK, edge, 9), slot


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_bank_and_context_as_they_were(engine_factory):
    eng = engine_factory(ws.FS, ws.N)
    lib, ctx, p = eng.lib, eng.ctx, _lib.ptr
    n = ws.N
    x = np.ascontiguousarray(ws.iq()[:40 * n])
    good = inits_of([(0, ws.inits()[0]), (0, ws.inits()[3])])
    bank = eng.create_weak_bank(good, None, 100)
    h = bank.handle
    ms = np.zeros((2, 40), dtype=_lib.WEAK_MS_REC)
    per = np.zeros((2, 3), dtype=_lib.WEAK_PERIOD_REC)
    cnt = np.zeros(2, dtype=np.int32)
    d_iq = eng.alloc(x.nbytes).upload(x)
    d_out = eng.alloc(ms.nbytes)
    before = bank.state().tobytes()

    def track(iq=x, n_streams=1, first=100, n_ms=40, bank=h):
        return lib.gyp_weak_track_block(bank, None if iq is None else p(iq), n_streams, first, n_ms, p(ms), p(per), p(cnt))

    def track_dev(iq=d_iq.ptr, stride=40 * n, first=100, n_ms=40, bank=h):
        return lib.gyp_weak_track_block_dev(bank, iq, stride, first, n_ms, d_out.ptr, None, None)

    def create(inits=good, n_chan=None, prm=None, first=0, **field):
        if field:
            prm = _records.WeakParams(**field).record()
        out = _lib.C.c_void_p()
        rc = lib.gyp_weak_bank_create(ctx, None if inits is None else p(inits), len(good) if n_chan is None else n_chan, p(prm), first, _lib.C.byref(out))
        assert not out.value
        return rc

    def init_with(**kw):
        a = good.copy()
        for k, v in kw.items():
            a[k][1] = v
        return a

    def state_with(**kw):
        st = np.zeros(1, dtype=_lib.WEAK_STATE)
        st["f"], st["f_int"], st["u0"], st["c0"], st["edge"] = 100.0, 100.0, 0.5, 5, 3
        for k, v in kw.items():
            st[k] = v
        return lib.gyp_weak_bank_set_state(h, 0, p(st))

    refusals = []
    for name, call in (("track", track), ("track_dev", track_dev)):
        refusals += [(name, "NULL samples", lambda c=call: c(iq=None)), (name, "n_ms = 0", lambda c=call: c(n_ms=0)), (name, "n_ms < 0", lambda c=call: c(n_ms=-20)),
                     (name, "n_ms > 65535", lambda c=call: c(n_ms=65536)), (name, "first_ms before the cursor", lambda c=call: c(first=99)),
                     (name, "first_ms after the cursor", lambda c=call: c(first=101)), (name, "first_ms 0", lambda c=call: c(first=0))]
    refusals += [("track", "no streams", lambda: track(n_streams=0)), ("track_dev", "a stride below n_ms N", lambda: track_dev(stride=40 * n - 1)),
                 ("create", "NULL inits", lambda: create(inits=None)), ("create", "no channels", lambda: create(n_chan=0)),
                 ("create", "negative count", lambda: create(n_chan=-1)), ("create", "first_ms < 0", lambda: create(first=-1)),
                 ("create", "satellite 0", lambda: create(inits=init_with(sat_id=0))), ("create", "satellite 33", lambda: create(inits=init_with(sat_id=33))),
                 ("create", "a negative stream", lambda: create(inits=init_with(stream=-1))),
                 ("create", "a NaN Doppler", lambda: create(inits=init_with(doppler_hz=np.nan))), ("create", "an infinite Doppler", lambda: create(inits=init_with(doppler_hz=np.inf))),
                 ("create", "a NaN carrier phase", lambda: create(inits=init_with(carrier_phase=np.nan))),
                 ("create", "period 10", lambda: create(period_ms=10)), ("create", "sync_ms 39", lambda: create(sync_ms=39)),
                 ("create", "sync_ms 2001", lambda: create(sync_ms=2001)), ("create", "spacing 0", lambda: create(spacing=0)),
                 ("create", "spacing above a chip", lambda: create(spacing=(1 << 40) + 1)), ("create", "PLL bandwidth 0", lambda: create(pll_bw_hz=0.0)),
                 ("create", "PLL bandwidth NaN", lambda: create(pll_bw_hz=float("nan"))), ("create", "PLL bandwidth 51", lambda: create(pll_bw_hz=51.0)),
                 ("create", "DLL bandwidth 0", lambda: create(dll_bw_hz=0.0)), ("create", "DLL bandwidth 11", lambda: create(dll_bw_hz=11.0)),
                 ("create", "lose_mu < 0", lambda: create(lose_mu=-0.5)), ("create", "lose_mu NaN", lambda: create(lose_mu=float("nan"))),
                 ("set_channel", "index 2", lambda: lib.gyp_weak_bank_set_channel(h, 2, p(good))), ("set_channel", "index -1", lambda: lib.gyp_weak_bank_set_channel(h, -1, p(good))),
                 ("set_channel", "NULL", lambda: lib.gyp_weak_bank_set_channel(h, 0, None)),
                 ("set_channel", "satellite 33", lambda: lib.gyp_weak_bank_set_channel(h, 0, p(init_with(sat_id=33)[1:]))),
                 ("set_channel", "NaN Doppler", lambda: lib.gyp_weak_bank_set_channel(h, 0, p(init_with(doppler_hz=np.nan)[1:]))),
                 ("drop_channel", "index 2", lambda: lib.gyp_weak_bank_drop_channel(h, 2)),
                 ("set_state", "u0 = 1", lambda: state_with(u0=1.0)), ("set_state", "c0 < 0", lambda: state_with(c0=-1)),
                 ("set_state", "c0 = 1023 chips", lambda: state_with(c0=wm.CODE_MOD)), ("set_state", "edge 20", lambda: state_with(edge=20)),
                 ("set_state", "NaN f", lambda: state_with(f=np.nan)), ("set_state", "index 2", lambda: lib.gyp_weak_bank_set_state(h, 2, p(np.zeros(1, dtype=_lib.WEAK_STATE))))]
    try:
        for name, what, call in refusals:
            assert call() == BAD_ARG, (name, what)
            assert lib.gyp_last_error(ctx), (name, what)
        # a stream format other than the one the bank was created under
        other = GypsumEngine(0)
        other.set_stream_format(ws.FS, ws.N)
        bank2 = other.create_weak_bank(good, None, 100)
        other.set_stream_format(2 * ws.FS, 2 * ws.N)
        assert lib.gyp_weak_track_block(bank2.handle, p(x), 1, 100, 20, p(ms), p(per), p(cnt)) == BAD_ARG
        assert b"stream format" in lib.gyp_last_error(other.ctx)
        # the host form alone: a channel on a stream that was not passed
        bank3 = eng.create_weak_bank(init_with(stream=1), None, 100)
        assert track(bank=bank3.handle) == BAD_ARG and b"stream" in lib.gyp_last_error(ctx)
        bank3.close()
        eng.sync()
        assert not ms.tobytes().strip(b"\0") and not per.tobytes().strip(b"\0") and not cnt.any()     # nothing ran, nothing was written
        assert bank.state().tobytes() == before and bank.cursor == 100 and bank2.cursor == 100
        bank2.close()
        other.close()
        # and the bank still runs: the same records as a bank nothing was refused on
        a = bank.track_block(x, 1, 100, 40)
        fresh = eng.create_weak_bank(good, None, 100)
        b = fresh.track_block(x, 1, 100, 40)
        assert a[0].tobytes() == b[0].tobytes() and bank.cursor == 140
        fresh.close()
    finally:
        d_iq.free()
        d_out.free()
        bank.close()


# ---------------------------------------------------------------------------------------------- end to end
def test_weak_search_then_tracker_gives_the_scenes_bits():
    from gypsum_amd.acquisition import GpsSatelliteDetector
    from gypsum_amd.antenna_sample_provider import SampleProviderAttributes
    from gypsum_amd.tracker import BitValue
    from gypsum_amd.weak_tracker import WeakSignalTracker
    attrs = SampleProviderAttributes(samples_per_second=ws.FS, samples_per_prn_transmission=ws.N)
    x = ws.iq()
    found = GpsSatelliteDetector({}).detect_weak_satellites_in_antenna_data(list(range(1, 33)), x[:220 * ws.N], attrs)
    ids = [f.satellite_id for f in found]
    assert set(ids) >= {7, 19, 26}
    tr = ws.truth()
    for sv in (7, 19, 26):                                             # the search lands on the nearer fine bin, as the model's did
        f = found[ids.index(sv)]
        assert abs(f.doppler_shift - tr[sv].doppler_hz) <= 5.0 and f.prn_phase_shift == tr[sv].code_phase, (sv, f.doppler_shift, f.prn_phase_shift)
    trk = WeakSignalTracker(found, attrs)
    events = trk.process(x[:1000 * ws.N]) + trk.process(x[1000 * ws.N:])
    for sv in (7, 19, 26):
        c = ids.index(sv)
        ev = [e for ch, e in events if ch == c]
        assert len(ev) >= 99
        starts = [round(e.receiver_timestamp * 1000) for e in ev]
        assert starts[0] % 20 == ws.true_edge(tr[sv]) and all(b - a == 20 for a, b in zip(starts, starts[1:]))
        assert all(e.receiver_timestamp == round(m * ws.N / ws.FS, 6) and e.trailing_edge_receiver_timestamp == round((m + 20) * ws.N / ws.FS, 6)
                   for e, m in zip(ev, starts))
        got = [1 if e.bit_value == BitValue.ONE else -1 for e in ev][ws.SETTLE_PERIODS:]
        want = [ws.true_bit(tr[sv], m) for m in starts][ws.SETTLE_PERIODS:]
        same = sum(int(g == w) for g, w in zip(got, want))
        assert same in (0, len(want)), (sv, same, len(want))        # every bit, up to the one sign a Costas loop leaves open
    status = trk.status()
    for sv in (7, 19, 26):
        s = status[ids.index(sv)]
        assert s.status == 0 and s.mu >= 4.0 and abs(s.doppler_hz - tr[sv].doppler_hz) < 3.0 and s.bit_edge == ws.true_edge(tr[sv])
        assert s.phase_rms < 0.35 and not s.false_lock, (sv, s.phase_rms)


def test_false_lock_from_the_farther_search_bin_is_flagged():
    """The loop's limit on the device as on the model (tests/test_weak_track_host.py): satellite 26 started 7 Hz off ends in a false
    lock that mu and status do not show and phase_rms does."""
    from gypsum_amd.acquisition import SatelliteAcquisitionAttemptResult
    from gypsum_amd.antenna_sample_provider import SampleProviderAttributes
    from gypsum_amd.weak_tracker import WeakSignalTracker
    attrs = SampleProviderAttributes(samples_per_second=ws.FS, samples_per_prn_transmission=ws.N)
    tr = ws.truth()
    sv, f = ws.FAR_BIN_STARTS[2]
    start = SatelliteAcquisitionAttemptResult(satellite_id=sv, doppler_shift=f, carrier_wave_phase_shift=0.3, prn_phase_shift=tr[sv].code_phase,
                                              correlation_strength=30.0)
    trk = WeakSignalTracker([start], attrs)
    assert math.isnan(trk.status()[0].phase_rms) and not trk.status()[0].false_lock
    trk.process(ws.iq())
    s = trk.status()[0]
    print(f"satellite {sv} from +7 Hz: mu {s.mu:.2f} phase rms {s.phase_rms:.3f} doppler {s.doppler_hz - tr[sv].doppler_hz:+.2f} Hz off")
    assert s.status == 0 and s.mu >= 4.0 and s.phase_rms > 0.7 and s.false_lock
