"""The exact code-loop sums with a stream's millisecond staged once for all its channels (gyp_debug_set "no_exact_shared").

Behind the throughput tracking kernel, at 8 samples per chip, dll_exact_shared_kernel groups the channels by stream on the device
and forms every channel's float64 prompt / early / late sums out of one float64 copy of the millisecond in LDS; with
"no_exact_shared" 1 every channel fetches and converts the samples itself (dll_exact_wave_kernel).  Same operands in the same
order: every case below runs with the switch at 0 and at 1 in one process and compares, with tobytes(), the track records, the
float64 discriminators (gyp_debug_disc_read) and gyp_bank_get_state.  "last_exact_path" is asserted in every case, so that
nothing passes through a silent fall-back.  All inputs are synthetic (generated on the device) except the fixture of the
lost-channel case.  The comparisons of this pass with the float64 oracle live in test_gpu_dll_exact.py, test_gpu_track_survey.py
and test_gpu_parity.py.
"""
from __future__ import annotations

import numpy as np
import pytest

import golden_util as gu
from gypsum_amd._lib import CHAN_INIT, SYNTH_SAT, TRACK_REC, GypsumHipError

pytestmark = pytest.mark.gpu

PATH_WAVE, PATH_SHARED = 1, 2


def _scene(rng, n_streams, n_sats, fs, same_ids=False):
    n = fs // 1000
    sats = np.zeros((n_streams, n_sats), dtype=SYNTH_SAT)
    for s in range(n_streams):
        sats[s]["sat_id"] = np.arange(1, n_sats + 1) if same_ids else rng.choice(np.arange(1, 33), size=n_sats, replace=False)
        sats[s]["code_phase"] = rng.integers(0, min(n, 2046), n_sats)
        sats[s]["doppler_hz"] = rng.uniform(-4500, 4500, n_sats)
        sats[s]["carrier_phase"] = rng.uniform(0, 2 * np.pi, n_sats)
        sats[s]["amplitude"] = 0.005 if n >= 8184 else 0.010
        sats[s]["nav_bit_offset_ms"] = rng.integers(0, 20, n_sats)
    return sats


def _init_of(scene, stream, k, code_phase=None):
    s = scene[stream, k]
    return (stream, int(s["sat_id"]), float(round(float(s["doppler_hz"]))), float(s["carrier_phase"]) + 0.1,
            int(s["code_phase"]) if code_phase is None else int(code_phase), 0)


class _Rig:
    """n_streams x n_ms of synthetic IQ and the start times in device memory."""

    def __init__(self, eng, fs, n_streams, n_ms, scene, seed, t_add=0.0):
        self.eng, self.fs, self.n, self.n_ms = eng, fs, fs // 1000, n_ms
        self.stride = n_ms * self.n
        self.iq = eng.alloc(n_streams * self.stride * 8)
        eng.synth_iq(self.iq, n_streams, self.stride, n_ms, scene, 0.03 if self.n >= 8184 else 0.05, seed)
        t = np.array([round(ms * self.n / fs, 6) + t_add for ms in range(n_ms)], dtype=np.float64)
        self.t_dev = eng.alloc(t.nbytes).upload(t)

    def block(self, bank, ms0, n_ms):
        """Track [ms0, ms0 + n_ms) on the device; (records, float64 discriminators, state), each as bytes."""
        eng = self.eng
        rec_dev = eng.alloc(bank.n_chan * n_ms * TRACK_REC.itemsize)
        bank.track_block_dev(self.iq.ptr.value + ms0 * self.n * 8, self.stride, n_ms, self.t_dev.ptr.value + ms0 * 8, rec_dev.ptr.value)
        eng.sync()
        rec = rec_dev.download(TRACK_REC, bank.n_chan * n_ms).reshape(bank.n_chan, n_ms)
        rec_dev.free()
        disc = bank.exact_discriminators(n_ms)
        st = bank.state()
        return rec, disc, b"".join(np.ascontiguousarray(st[k]).tobytes() for k in ("doppler_hz", "carrier_phase", "code_phase", "lost"))

    def free(self):
        self.iq.free()
        self.t_dev.free()


def _both(eng, run, want_shared=PATH_SHARED):
    """run() -> list of (records, discriminators, state) under either setting of the switch, on the throughput path; the results
    of "no_exact_shared" 0 after they have been found equal to those of 1."""
    out = {}
    eng.debug_set("no_spec", 1)
    try:
        for off in (1, 0):
            eng.debug_set("no_exact_shared", off)
            assert eng.debug_get("no_exact_shared") == off
            out[off] = run()
            assert eng.debug_get("last_exact_path") == (PATH_WAVE if off else want_shared), off
    finally:
        eng.debug_set("no_exact_shared", 0)
        eng.debug_set("no_spec", 0)
    assert len(out[0]) == len(out[1]) and len(out[0]) > 0
    for i, ((r0, d0, s0), (r1, d1, s1)) in enumerate(zip(out[0], out[1])):
        assert np.isfinite(d0).all(), i
        assert d0.tobytes() == d1.tobytes(), (i, "discriminators", int(np.sum(d0 != d1)))
        assert r0.tobytes() == r1.tobytes(), (i, "records")
        assert s0 == s1, (i, "state")
    return out[0]


def test_headline_shaped_bank_across_a_launch_boundary(engine_factory):
    """4 streams x 12 channels at 8.184 Msps, stream-major like the benchmark's bank, 320 ms: the tracking kernel goes through in
    a 250-ms and a 70-ms launch, the exact pass walks all 320 in one."""
    fs, n_streams, n_ms = 8_184_000, 4, 320
    eng = engine_factory(fs, fs // 1000)
    rng = np.random.default_rng(4120)
    scene = _scene(rng, n_streams, 12, fs)
    inits = np.array([_init_of(scene, s, k) for s in range(n_streams) for k in range(12)], dtype=CHAN_INIT)
    rig = _Rig(eng, fs, n_streams, n_ms, scene, 41)

    def run():
        bank = eng.create_bank(inits)
        got = rig.block(bank, 0, n_ms)
        bank.close()
        return [got]

    (rec, disc, _), = _both(eng, run)
    rig.free()
    assert not rec["status"].any()
    assert np.count_nonzero(disc) == disc.size


def test_any_channel_order_and_group_size(engine_factory):
    """Streams interleaved in the channel list; a stream with one channel, one with 13 and one with 17 (two groups each), one with
    five, a stream nobody tracks (index 3); one channel dropped before the block."""
    fs, n_streams, n_ms = 8_184_000, 5, 24
    eng = engine_factory(fs, fs // 1000)
    rng = np.random.default_rng(4121)
    scene = _scene(rng, n_streams, 17, fs, same_ids=True)
    per_stream = {0: 1, 1: 13, 2: 17, 4: 5}
    todo = {s: list(range(c)) for s, c in per_stream.items()}
    rows = []
    while any(todo.values()):                           # round-robin over the streams: neighbours in the list are on different streams
        for s in sorted(todo):
            if todo[s]:
                rows.append(_init_of(scene, s, todo[s].pop(0)))
    inits = np.array(rows, dtype=CHAN_INIT)
    assert len(inits) == 36 and len(set(inits["stream"][:4])) == 4
    dropped = 7
    rig = _Rig(eng, fs, n_streams, n_ms, scene, 42)

    def run():
        bank = eng.create_bank(inits)
        bank.drop_channel(dropped)
        got = rig.block(bank, 0, n_ms)
        bank.close()
        return [got]

    (rec, disc, _), = _both(eng, run)
    rig.free()
    assert np.all(rec[dropped]["status"] == 2) and not disc[dropped].any()
    others = np.arange(len(inits)) != dropped
    assert not rec[others]["status"].any() and np.count_nonzero(disc[others]) == disc[others].size


def test_groups_follow_the_device_state_after_reset_dev(engine_factory):
    """gyp_bank_reset_dev with a different channel-to-stream assignment between two blocks of one bank: the bank's host copy of the
    assignment is stale then, and the second block equals a fresh bank's only if the groups were built from the device state."""
    fs, n_streams, n_ms = 8_184_000, 3, 16
    eng = engine_factory(fs, fs // 1000)
    rng = np.random.default_rng(4122)
    scene = _scene(rng, n_streams, 17, fs, same_ids=True)
    n_chan = 24
    first = np.array([_init_of(scene, i % 3, i // 3) for i in range(n_chan)], dtype=CHAN_INIT)                  # 8 + 8 + 8, interleaved
    stream_b = [2] * 17 + [0] * 6 + [1]                                                                         # 17 + 6 + 1, in runs
    second = np.array([_init_of(scene, s, i if s == 2 else i - 17) for i, s in enumerate(stream_b)], dtype=CHAN_INIT)
    assert np.any(first["stream"] != second["stream"])
    rig = _Rig(eng, fs, n_streams, n_ms, scene, 43)
    second_dev = eng.alloc(second.nbytes).upload(second)

    def run():
        bank = eng.create_bank(first)
        a = rig.block(bank, 0, n_ms)
        bank.reset_dev(second_dev.ptr.value)
        b = rig.block(bank, 0, n_ms)
        bank.close()
        fresh = eng.create_bank(second)
        c = rig.block(fresh, 0, n_ms)
        fresh.close()
        for x, y in zip(b, c):                          # under THIS setting of the switch: re-assigned bank == fresh bank
            assert (x if isinstance(x, bytes) else x.tobytes()) == (y if isinstance(y, bytes) else y.tobytes())
        return [a, b, c]

    a, b, _ = _both(eng, run)
    rig.free()
    second_dev.free()
    assert a[0].tobytes() != b[0].tobytes()             # the two assignments really give different records


def test_every_sample_offset_and_the_cut_windows(engine_factory):
    """Code phases s = 8 * 37 + r for every r = s mod 8, and s = 0, 1, 7, 8176, 8183 (q = 0 and q = 1022: the windows cut by the
    ends of the circular block), at a start time of 40 s.  The first millisecond of each channel runs at exactly that lag."""
    fs, n_ms = 8_184_000, 4
    eng = engine_factory(fs, fs // 1000)
    rng = np.random.default_rng(4123)
    scene = _scene(rng, 1, 13, fs, same_ids=True)
    phases = [8 * 37 + r for r in range(8)] + [0, 1, 7, 8176, 8183]
    inits = np.array([_init_of(scene, 0, k, code_phase=s) for k, s in enumerate(phases)], dtype=CHAN_INIT)
    rig = _Rig(eng, fs, 1, n_ms, scene, 44, t_add=40.0)

    def run():
        bank = eng.create_bank(inits)
        got = rig.block(bank, 0, n_ms)
        bank.close()
        return [got]

    (rec, disc, _), = _both(eng, run)
    rig.free()
    assert not rec["status"].any() and np.count_nonzero(disc) == disc.size


def test_a_channel_lost_part_way(engine_factory):
    """tests/golden/track_8184_long.npz: the channel that starts 250 Hz off is dropped by the 6-second watchdog in the middle of a
    block; its later milliseconds (status 2) are skipped by either kernel."""
    z = gu.load("track_8184_long.npz")
    fs, n = int(z["fs"]), int(z["n"])
    eng = engine_factory(fs, n)
    iq = gu.tracking_iq(z)
    tracked = [int(s) for s in z["tracked"]]
    n_ms = int(z["n_ms"])
    inits = np.zeros(len(tracked), dtype=CHAN_INIT)
    for i, sv in enumerate(tracked):
        acq = z[f"acq_{sv}"]
        inits[i] = (0, sv, acq[0], acq[1], int(acq[2]), 0)
    lost = [i for i, sv in enumerate(tracked) if int(z[f"lost_{sv}"]) >= 0]
    assert lost, "the fixture is meant to lose a channel"
    t0 = np.array([gu.chunk_times(ms, n, fs)[0] for ms in range(9, n_ms)], dtype=np.float64)
    iq_dev = eng.alloc((n_ms - 9) * n * 8).upload(np.ascontiguousarray(iq[9 * n:n_ms * n], dtype=np.complex64))
    t_dev = eng.alloc(t0.nbytes).upload(t0)
    cuts = list(range(0, n_ms - 9, 3500)) + [n_ms - 9]

    def run():
        bank = eng.create_bank(inits)
        out = []
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            rec_dev = eng.alloc(bank.n_chan * (b1 - b0) * TRACK_REC.itemsize)
            bank.track_block_dev(iq_dev.ptr.value + b0 * n * 8, (n_ms - 9) * n, b1 - b0, t_dev.ptr.value + b0 * 8, rec_dev.ptr.value)
            eng.sync()
            rec = rec_dev.download(TRACK_REC, bank.n_chan * (b1 - b0)).reshape(bank.n_chan, b1 - b0)
            rec_dev.free()
            st = bank.state()
            out.append((rec, bank.exact_discriminators(b1 - b0),
                        b"".join(np.ascontiguousarray(st[k]).tobytes() for k in ("doppler_hz", "carrier_phase", "code_phase", "lost"))))
        bank.close()
        return out

    got = _both(eng, run)
    iq_dev.free()
    t_dev.free()
    rec = np.concatenate([g[0] for g in got], axis=1)
    for i in lost:
        at = int(z[f"lost_{tracked[i]}"]) - 9
        assert 0 < at < rec.shape[1] - 1 and at % 3500 not in (0, 3499)          # part-way through a block
        assert rec[i, at]["status"] == 1 and np.all(rec[i, at + 1:]["status"] == 2) and not rec[i, :at]["status"].any()


def test_two_samples_per_chip_keeps_the_per_channel_kernel(engine_factory):
    """2.046 Msps (K = 2): the staged form is built for 8 samples per chip only; either setting runs dll_exact_wave_kernel."""
    fs, n_streams, n_ms = 2_046_000, 2, 40
    eng = engine_factory(fs, fs // 1000)
    rng = np.random.default_rng(4124)
    scene = _scene(rng, n_streams, 6, fs)
    inits = np.array([_init_of(scene, k % 2, k // 2) for k in range(12)], dtype=CHAN_INIT)
    rig = _Rig(eng, fs, n_streams, n_ms, scene, 45)

    def run():
        bank = eng.create_bank(inits)
        got = rig.block(bank, 0, n_ms)
        bank.close()
        return [got]

    (rec, disc, _), = _both(eng, run, want_shared=PATH_WAVE)
    rig.free()
    assert not rec["status"].any() and np.count_nonzero(disc) == disc.size


def test_switch_is_range_checked_and_the_witness_read_only(engine_factory):
    eng = engine_factory(8_184_000, 8184)
    assert eng.debug_get("no_exact_shared") == 0
    for bad in (-1, 2, 0.5, float("nan")):
        with pytest.raises(GypsumHipError):
            eng.debug_set("no_exact_shared", bad)
    with pytest.raises(GypsumHipError):
        eng.debug_set("last_exact_path", 1)
    eng.debug_set("no_exact_shared", 1)
    assert eng.debug_get("no_exact_shared") == 1
    eng.debug_set("no_exact_shared", 0)
    bank = eng.create_bank(np.array([(0, 1, 0.0, 0.0, 0, 0)], dtype=CHAN_INIT))
    with pytest.raises(GypsumHipError):                 # no block tracked yet: nothing to read
        bank.exact_discriminators(10)
    bank.close()
