"""Bank slots that are re-used: gyp_bank_set_channel, gyp_bank_drop_channel and gyp_bank_reset_dev on banks WITH a history.

A receiver parks slots, revives one with a new acquisition, drops it, revives it again (gypsum_amd/receiver.py), and bench.py resets
a used bank before every timed step.  bank_reset_kernel and set_channel leave the rings of the previous life in place (err_ring,
peak_re, peak_im) and rely on every reader bounding itself by n_steps; here the previous life is long enough for that to matter: more
than 1000 peaks (the ring has wrapped), past the 1024-ms refresh, a full 250-ms lock window and locked = 1 at its end.

Every case runs on each tracking path that can take it -- all seven of PATHS, except that the goldens of case 4 exist at 2.046 and
8.184 Msps only and case 6 is about the shared exact kernel's grouping by stream -- and asserts the path (PATHS: the speculative tracker's sub-block count and
fast-path records, "last_exact_path" on the throughput kernel, no fast-path record under gyp_bank_keep_profiles).  Every life is compared
  * with a fresh float64 orc.Tracker given the same init and the same chunk times (test_gpu_params._assert_same's criteria: status,
    code phase, peak offset, pseudosymbol, locked exact; Doppler within 1e-3 Hz; |peak| within RTOL_MAG), and
  * with a FRESH bank created from the same inits and fed the same blocks on the same path: byte equality of the records, of
    gyp_bank_get_state and, on the throughput path, of gyp_debug_disc_read.  (A fresh bank run twice gives the same bytes on every
    path, the speculative one included: _fresh_twice asserts it before anything is compared with it.)
The scenes' lock verdicts are no knife edges in the oracle (relative margin > 1e-4, asserted), so an exact lock flag is a fair demand.
"""
from __future__ import annotations

import numpy as np
import pytest

import golden_util as gu
import receiver_model as rm
from gypsum_amd import _lib, synth
from gypsum_amd._lib import CHAN_INIT, GypsumHipError
from oracle import gypsum_oracle as orc

pytestmark = pytest.mark.gpu

RTOL_MAG = 1e-4           # tests/test_gpu_parity.py: float32 transform against the float64 one
MIN_LOCK_MARGIN = 1e-4    # well above the documented float32 floor of the lock verdicts (1e-7 .. 3e-5)
FIRST_LIFE_MS, SECOND_LIFE_MS, BLOCK_MS = 1300, 600, 500

# name -> (fs, debug switches, kind, expected "last_exact_path"); kind: "spec" speculative tracker, "thr" throughput kernel,
# "prof" gyp_bank_keep_profiles (transform kernel)
PATHS = {
    "spec-K2": (2_046_000, {}, "spec", None),
    "spec-K8": (8_184_000, {"spec_sub_ms": 200}, "spec", None),          # 500-ms blocks in more than one sub-block at this rate too
    "thr-K8-shared": (8_184_000, {"no_spec": 1}, "thr", 2),
    "thr-K8-wave": (8_184_000, {"no_spec": 1, "no_exact_shared": 1}, "thr", 1),
    "thr-K2": (2_046_000, {"no_spec": 1}, "thr", 1),
    "thr-K16": (16_368_000, {"no_spec": 1}, "thr", 3),
    "prof-K2": (2_046_000, {}, "prof", None),
}
SCENE_SEED = {2_046_000: 0, 8_184_000: 0, 16_368_000: 3}     # chosen with the oracle so that _Scene.check() holds: smallest lock margins 5.9e-3, 1.8e-4, 4.1e-4


# ---------------------------------------------------------------- the oracle side, once per rate
def _acq(sat, dop, phi, cp):
    return orc.AcquisitionResult(int(sat), dop, float(phi), int(cp), 0.0)


def _oracle_lives(iq, fs, jobs, consts=None):
    """jobs: (sat_id, doppler, carrier phase, code phase, first step, end step) -> rm.Life each, in worker processes."""
    n = fs // 1000
    consts = dict(rm._constants(), **(consts or {}))
    with rm.shared_samples(iq, len(jobs)) as (path, pool):
        return pool.map(rm.life_job, [(path, fs, n, _acq(*j[:4]), j[4], j[5], consts) for j in jobs])


class _Scene:
    """Three satellites A, B, C in the firm-lock part of synth.lock_regime_scene's ranges, 1900 ms.  The bank tracks A (slot 0) and B
    (slot 1) from millisecond 0; at 1300 slot 0 starts a second life on C."""

    def __init__(self, fs):
        self.fs, self.n = fs, fs // 1000
        self.n_ms = FIRST_LIFE_MS + SECOND_LIFE_MS
        scene = synth.random_scene(fs, self.n_ms, 3, 7100 + SCENE_SEED[fs], max_code_phase=(2046 if self.n > 2046 else None),
                                   amplitude=22.0 / self.n, noise_sigma=float(np.sqrt(0.3 / self.n)))
        self.iq = synth.render(scene)
        self.t0 = np.array([orc.chunk_times(ms * self.n, self.n, fs)[0] for ms in range(self.n_ms)])
        self.init = [(0, s.sat_id, float(int(round(s.doppler_hz)) + 1), float(s.carrier_phase) + 0.1, int(s.code_phase), 0) for s in scene.sats]
        a, b, c = self.init
        jobs = [(a[1], a[2], a[3], a[4], 0, FIRST_LIFE_MS), (b[1], b[2], b[3], b[4], 0, self.n_ms), (c[1], c[2], c[3], c[4], FIRST_LIFE_MS, self.n_ms),
                (a[1], a[2], a[3], a[4], 0, self.n_ms)]
        self.life_a, self.life_b, self.life_c, self.life_a_whole = _oracle_lives(self.iq, fs, jobs)

    def check(self):
        """Conditions on the oracle alone: A is locked at the end of its first life; C's life cannot lock during its first 249 ms and
        locks later; no lock verdict is a knife edge."""
        assert self.life_a.records[-1].locked and len(self.life_a.records) == FIRST_LIFE_MS
        c = self.life_c.records
        assert len(c) == SECOND_LIFE_MS and not any(r.locked for r in c[:249]) and any(r.locked for r in c[249:])
        worst = min(l.min_lock_margin for l in (self.life_a_whole, self.life_b, self.life_c))
        print(f"[bank lifecycle {self.fs / 1e6:.3f} Msps] smallest lock margin of the oracle lives {worst:.3e}")
        assert worst > MIN_LOCK_MARGIN
        assert all(l.lost_at is None for l in (self.life_a_whole, self.life_b, self.life_c))


_scenes = {}


def _scene(fs) -> _Scene:
    if fs not in _scenes:
        _scenes[fs] = _Scene(fs)
        _scenes[fs].check()
    return _scenes[fs]


def _same_as_oracle(rec, life, nudged=False):
    """One channel's records from the life's first millisecond on, against the oracle's (test_gpu_params._assert_same)."""
    rows = life.records
    g = rec[:len(rows)]
    assert len(g) == len(rows)
    assert not g["status"].any()
    for name, want in (("code_phase", [r.code_phase_after for r in rows]), ("peak_offset", [r.peak_offset for r in rows]),
                       ("pseudosymbol", [r.pseudosymbol for r in rows]), ("locked", [int(r.locked) for r in rows])):
        bad = np.flatnonzero(g[name].astype(np.int64) != np.array(want, dtype=np.int64))
        assert bad.size == 0, (name, "first at millisecond", int(bad[0]), int(g[name][bad[0]]), want[bad[0]], bad.size)
    assert np.abs(g["doppler_hz"] - np.array([r.doppler_after for r in rows])).max() < 1e-3
    mag = np.abs(np.array([r.peak for r in rows]))
    assert np.all(np.abs(np.hypot(g["peak_re"].astype(np.float64), g["peak_im"].astype(np.float64)) - mag) <= RTOL_MAG * mag)
    if nudged:
        assert [bool(v) for v in g["nudged"]] == [bool(r.nudged) for r in rows]
    if life.lost_at is not None and len(rec) > len(rows):
        assert int(rec[len(rows)]["status"]) == 1


# ---------------------------------------------------------------- the device side
def _state_bytes(st):
    return b"".join(np.ascontiguousarray(st[k]).tobytes() for k in ("doppler_hz", "carrier_phase", "code_phase", "lost"))


class _Path:
    """A tracking path held for the length of a `with`: its switches set, then put back whatever happens."""

    def __init__(self, engine_factory, name):
        self.name = name
        self.fs, self.switches, self.kind, self.exact = PATHS[name]
        self.n = self.fs // 1000
        self.eng = engine_factory(self.fs, self.n)

    def __enter__(self):
        self.old = {k: self.eng.debug_get(k) for k in self.switches}
        for k, v in self.switches.items():
            self.eng.debug_set(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.eng.debug_set(k, v)
        return False

    def run(self, iq, t0, inits, ops, n_streams=1):
        """A new bank, then `ops` in order; returns one (records, state bytes, discriminators or None) per tracked block.
        ops: ("track", ms0, ms1) | ("set", slot, init) | ("drop", slot) | ("reset", inits) | ("refused", callable on the bank)."""
        eng, n = self.eng, self.n
        iq = np.asarray(iq).reshape(n_streams, -1)
        bank = eng.create_bank(np.array(inits, dtype=CHAN_INIT))
        out = []
        try:
            if self.kind == "prof":
                bank.keep_profiles(8)
            for op in ops:
                if op[0] == "track":
                    _, a, b = op
                    rec = bank.track_block(iq[:, a * n:b * n], n_streams, b - a, t0[a:b])
                    self._witness(bank, rec, b - a)
                    out.append((rec, _state_bytes(bank.state()), bank.exact_discriminators(b - a) if self.kind == "thr" else None))
                elif op[0] == "set":
                    bank.set_channel(op[1], op[2])
                elif op[0] == "drop":
                    bank.drop_channel(op[1])
                elif op[0] == "reset":
                    dev = eng.alloc(len(op[1]) * CHAN_INIT.itemsize).upload(np.array(op[1], dtype=CHAN_INIT))
                    bank.reset_dev(dev.ptr.value)
                    eng.sync()
                    dev.free()
                elif op[0] == "refused":
                    with pytest.raises(GypsumHipError) as e:
                        op[1](bank)
                    assert e.value.code == -1            # GYP_E_BAD_ARG
                else:
                    raise ValueError(op[0])
            self.last_profiles = [bank.profiles(i) for i in range(bank.n_chan)] if self.kind == "prof" else None
        finally:
            bank.close()
        return out

    def _witness(self, bank, rec, n_ms):
        """The block really ran on the path this case is named after."""
        live = rec["status"] == 0
        fast = (rec["path_info"] & 3) == 1
        if self.kind == "spec":
            stats = np.zeros(4, dtype=np.int32)
            self.eng._check(self.eng.lib.gyp_debug_spec_redo_read(bank.handle, _lib.ptr(stats)))
            assert stats[0] > (1 if n_ms >= 400 else 0), (self.name, stats)
            assert fast[live].any() or n_ms < 20 or not live.any(), self.name
        else:
            assert not fast.any(), self.name
            if self.kind == "thr":
                assert self.eng.debug_get("last_exact_path") == self.exact, self.name


def _equal_blocks(got, want, what, channels=None):
    assert len(got) == len(want)
    for k, ((r0, s0, d0), (r1, s1, d1)) in enumerate(zip(got, want)):
        if channels is None:
            assert r0.tobytes() == r1.tobytes(), (what, "records of block", k)
            assert s0 == s1, (what, "state after block", k)
            assert (d0 is None) == (d1 is None) and (d0 is None or d0.tobytes() == d1.tobytes()), (what, "discriminators of block", k)
        else:
            for c in channels:
                assert r0[c].tobytes() == r1[c].tobytes(), (what, "records of block", k, "channel", c)
                assert d0 is None or d0[c].tobytes() == d1[c].tobytes(), (what, "discriminators of block", k, "channel", c)


def _fresh_twice(path, iq, t0, inits, ops, n_streams=1):
    """A fresh bank's run, after a second one has given the same bytes."""
    a = path.run(iq, t0, inits, ops, n_streams)
    _equal_blocks(path.run(iq, t0, inits, ops, n_streams), a, "a fresh bank run twice")
    return a


def _blocks(a, b):
    cuts = list(range(a, b, BLOCK_MS)) + [b]
    return [("track", x, y) for x, y in zip(cuts[:-1], cuts[1:])]


def _channel_state(state_bytes, n_chan, c):
    """Channel c's four entries out of _state_bytes."""
    f = np.frombuffer(state_bytes[:16 * n_chan], dtype=np.float64).reshape(2, n_chan)
    i = np.frombuffer(state_bytes[16 * n_chan:], dtype=np.int32).reshape(2, n_chan)
    return f[:, c].tobytes() + i[:, c].tobytes()


# ---------------------------------------------------------------- 1, 2: re-use after a long history; neighbours untouched
@pytest.mark.parametrize("name", list(PATHS))
def test_a_slot_with_a_long_history_starts_a_new_life_like_a_fresh_bank(engine_factory, name):
    """Slot 0 tracks A for 1300 ms in blocks of 500 (locked at the end), then C for 600 ms, started (a) by set_channel, (b) by
    reset_dev of the whole bank, (c) by drop_channel, one block, set_channel (there A's life is 1299 ms and the block in between is
    millisecond 1299).  C's life cannot lock before its own 250th millisecond: sums or ring entries left by A's locked life would show."""
    fs = PATHS[name][0]
    sc = _scene(fs)
    a, b, c = sc.init
    first, second = _blocks(0, FIRST_LIFE_MS), _blocks(FIRST_LIFE_MS, sc.n_ms)
    first_c, gap = _blocks(0, FIRST_LIFE_MS - 1), ("track", FIRST_LIFE_MS - 1, FIRST_LIFE_MS)
    with _Path(engine_factory, name) as path:
        fresh = _fresh_twice(path, sc.iq, sc.t0, [c, b], second)                # the second life alone, on a new bank
        untouched = {False: path.run(sc.iq, sc.t0, [a, b], first + second),    # no slot re-used, in either way's blocks
                     True: path.run(sc.iq, sc.t0, [a, b], first_c + [gap] + second)}
        ways = {
            "set_channel": first + [("set", 0, c)] + second,
            "reset_dev": first + [("reset", [c, b])] + second,
            "drop_channel, a block, set_channel": first_c + [("drop", 0), gap, ("set", 0, c)] + second,
        }
        for way, ops in ways.items():
            dropping = way.startswith("drop")
            got = path.run(sc.iq, sc.t0, [a, b], ops)
            ref = untouched[dropping]
            assert len(got) == len(ref)
            n_first = len(first_c) if dropping else len(first)
            life1 = np.concatenate([g[0] for g in got[:n_first]], axis=1)
            assert life1[0, -1]["locked"] == 1, way                           # the history the new life must not see
            _same_as_oracle(life1[0], rm.Life(a[1], 0, None, sc.life_a.records[:life1.shape[1]]))
            _equal_blocks(got[:n_first], ref[:n_first], way + ": before the re-use")
            tail = got[-len(second):]
            life2 = np.concatenate([g[0] for g in tail], axis=1)
            _same_as_oracle(life2[0], sc.life_c)
            assert not life2[0, :249]["locked"].any() and life2[0, 249:]["locked"].any(), way
            if way == "reset_dev":                                             # the whole bank restarted, B too: a fresh bank's bytes
                _equal_blocks(tail, fresh, way)
                continue
            _equal_blocks(tail, fresh, way, channels=[0])                      # slot 0 is the fresh bank's ...
            for t, f in zip(tail, fresh):
                assert _channel_state(t[1], 2, 0) == _channel_state(f[1], 2, 0), way
            _equal_blocks(got, ref, way + ": the neighbour", channels=[1])     # ... and B never noticed
            for g, u in zip(got, ref):
                assert _channel_state(g[1], 2, 1) == _channel_state(u[1], 2, 1), way
            _same_as_oracle(np.concatenate([g[0][1] for g in got]), sc.life_b)
            if dropping:
                parked = got[n_first]
                assert np.all(parked[0][0]["status"] == 2) and (parked[2] is None or not parked[2][0].any())
                assert _channel_state(parked[1], 2, 0)[:-4] == _channel_state(got[n_first - 1][1], 2, 0)[:-4]      # frozen bit for bit
                assert _channel_state(parked[1], 2, 0)[-4:] == np.int32(1).tobytes()                               # and reads lost


# ---------------------------------------------------------------- 3: the watchdog clock of a new life, short period
WATCHDOG_VARIANTS = {
    "looks": {"watchdog_period_s": 0.3},
    "nudges": {"watchdog_period_s": 0.3, "watchdog_drop_below": 0.02, "watchdog_nudge_below": 0.995, "watchdog_nudge_hz": 3.0},
}
ORACLE_NAME = {"watchdog_period_s": "WATCHDOG_PERIOD_S", "watchdog_drop_below": "WATCHDOG_DROP_BELOW",
               "watchdog_nudge_below": "WATCHDOG_NUDGE_BELOW", "watchdog_nudge_hz": "WATCHDOG_NUDGE_HZ"}
_watchdog_lives = {}


def _watchdog_oracle(sc, variant, start):
    key = (sc.fs, variant, start)
    if key not in _watchdog_lives:
        a, b, c = sc.init
        consts = {ORACLE_NAME[k]: v for k, v in WATCHDOG_VARIANTS[variant].items()}
        jobs = [(b[1], b[2], b[3], b[4], 0, sc.n_ms), (c[1], c[2], c[3], c[4], start, sc.n_ms)]
        _watchdog_lives[key] = _oracle_lives(sc.iq, sc.fs, jobs, consts)
    return _watchdog_lives[key]


@pytest.mark.parametrize("variant", list(WATCHDOG_VARIANTS))
@pytest.mark.parametrize("name", list(PATHS))
def test_a_new_life_starts_its_watchdog_clock_at_zero(engine_factory, name, variant):
    """watchdog_period_s = 0.3 (oracle patched alike).  Slot 0 starts C at t = 0.32 s: a new tracker's clock is 0 (tracker.py:222), so
    its FIRST millisecond is a look, at one peak, where get_iq_constellation_circularity returns None and only the clock is stamped
    (tracker.py:370-376, utils.py:134-137); the later looks then fall every 0.3 s from THAT stamp, at 301, 601, 902 ... peaks (the
    reference stamps the clock on a None as well, so there is no look at two peaks; 902 because 1.22 - 0.92 < 0.3 in binary).  nudged, status and Doppler follow the oracle through
    all of them, with the reference's thresholds and with thresholds that make the later looks nudge."""
    start = 320
    sc = _scene(PATHS[name][0])
    a, b, c = sc.init
    life_b, life_c = _watchdog_oracle(sc, variant, start)
    looks = [(lk.step - start + 1, lk.n_peaks, lk.circularity, lk.action) for lk in life_c.looks]
    print(f"[watchdog of a new life, {variant}] looks of the second life (millisecond, peaks, circularity, action): {looks}")
    assert looks[0][:2] == (1, 1) and looks[0][2] is None and looks[0][3] == "none"
    assert len(looks) >= 4 and all(0 < lk[1] - 300 * k <= 3 for k, lk in enumerate(looks[1:4], 1))
    for lk in (l for life in (life_b, life_c) for l in life.looks if l.circularity is not None):      # no knife edge among the looks
        for thr in (WATCHDOG_VARIANTS[variant].get("watchdog_drop_below", 0.2), WATCHDOG_VARIANTS[variant].get("watchdog_nudge_below", 0.93)):
            assert abs(lk.circularity - thr) >= 1e-3, lk
    assert min(life_b.min_lock_margin, life_c.min_lock_margin) > MIN_LOCK_MARGIN
    if variant == "nudges":
        assert any(lk[3] == "nudge" for lk in looks[1:])
    with _Path(engine_factory, name) as path:
        old = path.eng.get_params()
        try:
            path.eng.set_params(**WATCHDOG_VARIANTS[variant])
            ops = [("track", 0, start), ("set", 0, c)] + _blocks(start, sc.n_ms)
            got = path.run(sc.iq, sc.t0, [a, b], ops)
            fresh = _fresh_twice(path, sc.iq, sc.t0, [c, b], _blocks(start, sc.n_ms))
        finally:
            path.eng.set_params(**old)
    tail = np.concatenate([g[0] for g in got[1:]], axis=1)
    _same_as_oracle(tail[0], life_c, nudged=True)
    _same_as_oracle(np.concatenate([g[0][1] for g in got]), life_b, nudged=True)
    _equal_blocks(got[1:], fresh, variant, channels=[0])


# ---------------------------------------------------------------- 4: the same at the default 6 s, on the goldens
_golden_cases = {}


def _golden_case(tag):
    """The fixture, the revival and the oracle's revived life, once per rate."""
    if tag in _golden_cases:
        return _golden_cases[tag]
    z = gu.load(f"track_{tag}_long.npz")
    fs, n, n_ms = int(z["fs"]), int(z["n"]), int(z["n_ms"])
    iq = gu.tracking_iq(z)
    tracked = [int(s) for s in z["tracked"]]
    inits = []
    for sv in tracked:
        acq = z[f"acq_{sv}"]
        inits.append((0, sv, float(acq[0]), float(acq[1]), int(acq[2]), 0))
    lost = [i for i, sv in enumerate(tracked) if int(z[f"lost_{sv}"]) >= 0]
    assert len(lost) == 1
    slot = lost[0]
    lost_at = int(z[f"lost_{tracked[slot]}"])
    healthy = tracked[(slot + 1) % len(tracked)]
    revive = lost_at + 101
    assert revive + 250 <= n_ms
    chips = orc.generate_ca_codes()
    a = orc.acquire_satellite(healthy, iq[(revive - 9) * n:(revive + 1) * n], fs, n, orc.prn_as_complex(chips[healthy - 1], n))
    assert a.correlation_strength > orc.ACQUISITION_STRENGTH_THRESHOLD + 1e-3
    new = (0, healthy, float(a.doppler_shift), float(a.carrier_wave_phase_shift), int(a.prn_phase_shift), 0)
    life, = _oracle_lives(iq, fs, [(healthy, new[2], new[3], new[4], revive, n_ms)])
    assert life.min_lock_margin > MIN_LOCK_MARGIN and life.lost_at is None
    assert (life.looks[0].step, life.looks[0].n_peaks, life.looks[0].circularity) == (revive, 1, None) and len(life.looks) == 1
    t0 = np.array([gu.chunk_times(ms, n, fs)[0] for ms in range(n_ms)])
    assert t0[revive] >= orc.WATCHDOG_PERIOD_S
    _golden_cases[tag] = (fs, n_ms, iq, t0, inits, slot, lost_at, revive, new, life)
    return _golden_cases[tag]


# every path at a rate that has a long golden: there is none at 16.368 Msps, so thr-K16 cannot take this case (case 3 gives it a new
# life's first look and the later ones)
@pytest.mark.parametrize("name", [k for k, v in PATHS.items() if v[0] in (2_046_000, 8_184_000)])
def test_a_lost_slot_is_revived_after_the_six_second_mark(engine_factory, name):
    """tests/golden/track_<rate>_long.npz (the reference's own run): the mis-tuned channel is dropped at the fixture's millisecond;
    one block later its slot is revived with the oracle's acquisition of a healthy satellite on the ten milliseconds that end at the
    revival step.  The new life starts beyond t = 6 s: its first millisecond is its first look."""
    fs, n_ms, iq, t0, inits, slot, lost_at, revive, new, life = _golden_case({2_046_000: "2046", 8_184_000: "8184"}[PATHS[name][0]])
    ops = _blocks(9, lost_at + 1) + [("track", lost_at + 1, revive), ("set", slot, new)] + _blocks(revive, n_ms)
    k_loss = len(_blocks(9, lost_at + 1)) - 1
    with _Path(engine_factory, name) as path:
        got = path.run(iq, t0, inits, ops)
        fresh_inits = list(inits)
        fresh_inits[slot] = new
        fresh = _fresh_twice(path, iq, t0, fresh_inits, _blocks(revive, n_ms))
    at_loss, parked = got[k_loss], got[k_loss + 1]
    assert at_loss[0][slot, -1]["status"] == 1 and not at_loss[0][slot, :-1]["status"].any()
    assert _channel_state(at_loss[1], len(inits), slot)[-4:] == np.int32(1).tobytes()
    assert np.all(parked[0][slot]["status"] == 2)
    assert _channel_state(parked[1], len(inits), slot) == _channel_state(at_loss[1], len(inits), slot)
    assert parked[2] is None or not parked[2][slot].any()
    tail = got[k_loss + 2:]
    _same_as_oracle(np.concatenate([g[0][slot] for g in tail]), life, nudged=True)
    _equal_blocks(tail, fresh, "revived slot", channels=[slot])
    for t, f in zip(tail, fresh):
        assert _channel_state(t[1], len(inits), slot) == _channel_state(f[1], len(inits), slot)


# ---------------------------------------------------------------- 5: drop_channel in mid-run
def _inline_oracle(sc, init, first, end, keep=0):
    """One channel through the oracle in this process (short runs); (records, its last `keep` prompt profiles)."""
    trk = orc.Tracker(orc.TrackingState(init[2], init[3], init[4]), orc.prn_as_complex(orc.generate_ca_codes()[init[1] - 1], sc.n), sc.fs, sc.n)
    rows = [trk.process_samples(sc.iq[ms * sc.n:(ms + 1) * sc.n], *orc.chunk_times(ms * sc.n, sc.n, sc.fs)) for ms in range(first, end)]
    return rows, list(trk.s.non_coherent_correlation_profiles)[-keep:] if keep else []


@pytest.mark.parametrize("name", list(PATHS))
def test_drop_in_mid_run_and_a_restart_of_a_live_channel(engine_factory, name):
    """Blocks of 60 ms: after the first, slot 0 is dropped (status 2 from then on, state frozen bit for bit, dropping it again is
    harmless); after the second, the LIVE slot 1 is restarted by set_channel on C and equals a fresh bank from that block on.  With
    gyp_bank_keep_profiles on, the rows of the live channel are still the oracle's."""
    sc = _scene(PATHS[name][0])
    a, b, c = sc.init
    ops = [("track", 0, 60), ("drop", 0), ("track", 60, 120), ("drop", 0), ("set", 1, c), ("track", 120, 180), ("track", 180, 240)]
    with _Path(engine_factory, name) as path:
        got = path.run(sc.iq, sc.t0, [a, b], ops)
        profiles = path.last_profiles
        fresh = _fresh_twice(path, sc.iq, sc.t0, [a, c], [("drop", 0), ("track", 120, 180), ("track", 180, 240)])
        if path.kind == "prof":                    # the rows right after the block in which slot 0 was parked
            path.run(sc.iq, sc.t0, [a, b], ops[:3])
            parked_profiles = path.last_profiles
    for g in got[1:]:
        assert np.all(g[0][0]["status"] == 2) and (g[2] is None or not g[2][0].any())
        assert _channel_state(g[1], 2, 0)[:-4] == _channel_state(got[0][1], 2, 0)[:-4]
        assert _channel_state(g[1], 2, 0)[-4:] == np.int32(1).tobytes()
    _same_as_oracle(np.concatenate([g[0][0] for g in got[:1]]), rm.Life(a[1], 0, None, _inline_oracle(sc, a, 0, 60)[0]))
    rows_b, prof_b = _inline_oracle(sc, b, 0, 120, keep=8)
    _same_as_oracle(np.concatenate([g[0][1] for g in got[:2]]), rm.Life(b[1], 0, None, rows_b))
    rows_c, prof_c = _inline_oracle(sc, c, 120, 240, keep=8)
    _same_as_oracle(np.concatenate([g[0][1] for g in got[2:]]), rm.Life(c[1], 120, None, rows_c))
    _equal_blocks(got[2:], fresh, "a live channel restarted", channels=[1])
    for g, f in zip(got[2:], fresh):
        assert _channel_state(g[1], 2, 1) == _channel_state(f[1], 2, 1)
    if profiles is not None:
        for rows, want in ((parked_profiles[1], prof_b), (profiles[1], prof_c)):
            assert rows.shape == (8, sc.n)
            for r, w in zip(rows, want):
                np.testing.assert_allclose(r, w, rtol=0, atol=1e-4 * float(w.max()))       # tests/test_gpu_profiles.py's bound


# ---------------------------------------------------------------- 6: set_channel to another stream, shared exact path
def test_set_channel_to_another_stream_regroups_the_shared_exact_pass(engine_factory):
    """Two streams at 8.184 Msps on the throughput kernel ("last_exact_path" 2: dll_exact_shared_kernel groups the channels by
    stream).  Between two blocks slot 0 moves from stream 0 to stream 1 (the same samples delayed by 50 ms, so another input at every
    millisecond): its records are a fresh bank's, and the host form still refuses a block that lacks the stream it now reads."""
    name = "thr-K8-shared"
    sc = _scene(PATHS[name][0])
    a, b, c = sc.init
    n, n_ms, shift = sc.n, 121, 50
    two = np.stack([sc.iq[:n_ms * n], sc.iq[shift * n:(shift + n_ms) * n]])
    moved = (1, c[1], c[2], c[3], c[4], 0)
    with _Path(engine_factory, name) as path:
        got = path.run(two, sc.t0, [a, b], [("track", 0, 60), ("set", 0, moved), ("track", 60, 120),
                                            ("refused", lambda bank: bank.track_block(two[:1, :n], 1, 1, sc.t0[120:121])),
                                            ("set", 0, (0,) + moved[1:]), ("track", 120, 121)], n_streams=2)
        fresh = _fresh_twice(path, two, sc.t0, [moved, b], [("track", 60, 120)], n_streams=2)
    _equal_blocks(got[1:2], fresh, "moved to stream 1", channels=[0])
    assert _channel_state(got[1][1], 2, 0) == _channel_state(fresh[0][1], 2, 0)
    trk = orc.Tracker(orc.TrackingState(c[2], c[3], c[4]), orc.prn_as_complex(orc.generate_ca_codes()[c[1] - 1], n), sc.fs, n)
    rows = [trk.process_samples(two[1, ms * n:(ms + 1) * n], *orc.chunk_times(ms * n, n, sc.fs)) for ms in range(60, 120)]
    _same_as_oracle(got[1][0][0], rm.Life(c[1], 60, None, rows))
    rows_b, _ = _inline_oracle(sc, b, 0, 120)
    _same_as_oracle(np.concatenate([g[0][1] for g in got[:2]]), rm.Life(b[1], 0, None, rows_b))
    assert not got[2][0]["status"].any()


# ---------------------------------------------------------------- 7: refused calls change nothing
@pytest.mark.parametrize("name", list(PATHS))
def test_refused_calls_change_nothing(engine_factory, name):
    sc = _scene(PATHS[name][0])
    a, b, c = sc.init
    refused = [("refused", lambda bank: bank.set_channel(-1, c)), ("refused", lambda bank: bank.set_channel(2, c)),
               ("refused", lambda bank: bank.drop_channel(-1)), ("refused", lambda bank: bank.drop_channel(2)),
               ("refused", lambda bank: bank.set_channel(0, (0, 0) + c[2:])), ("refused", lambda bank: bank.set_channel(0, (0, 33) + c[2:])),
               ("refused", lambda bank: bank.set_channel(1, (-1,) + c[1:]))]
    with _Path(engine_factory, name) as path:
        plain = _fresh_twice(path, sc.iq, sc.t0, [a, b], [("track", 0, 60), ("track", 60, 120)])
        got = path.run(sc.iq, sc.t0, [a, b], [("track", 0, 60)] + refused + [("track", 60, 120)])
    _equal_blocks(got, plain, "after refused calls")
