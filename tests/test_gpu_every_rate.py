"""Every stream rate against the float64 oracle: K x 1.023 Msps for K in GYP_FOR_EACH_RATE, the rates the resampler and the
down-converter hand real recordings to.

The surveys of tests/test_gpu_track_survey.py hold the closed-loop tracker and the 10-level acquisition at the reference's
recording rates (K = 2, 4, 8, 16).  The other rates run the same loops behind other staging schemes (kernels_common.hpp):
halo staging at K = 1, 3, 5, 6 (each thread also wipes the next chip's K - 1 samples, the last chip wraps to chip 0), own
staging with a ragged chip count per thread at K = 10, 12, general staging at K = 20, 48 (several rows per round) -- and the
float64 code loop (dll_exact_wave_kernel / dll_exact_block_kernel + dll_scan_kernel) re-runs behind each of them.  Here:
  * one multi-stream bank per rate (pull-in and lock-regime scenes side by side, launch cuts inside the block) with the bars of
    test_bench_shaped_banks_against_the_oracle;
  * code phases at and beyond N at K = 1 and 2 (the reference's DLL modulus is 2046 whatever N is);
  * the full-sky acquisition at every rate, noise-only satellites included;
  * strided, NaN-guarded device layouts give the packed host form's bits at every rate.
"""
from __future__ import annotations

import ctypes as C
import multiprocessing as mp
import time

import numpy as np
import pytest

import survey_worker
from gypsum_amd import _lib, synth
from oracle import gypsum_oracle as orc
from test_gpu_dll_exact import _engine_with_env
from test_gpu_track_survey import SEED_OFFSET, _bank_specs, _multi_stream_survey

RATES = [1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 48]


# ------------------------------------------------------------------ 1. one multi-stream bank per rate
# (K, pull-in scenes, satellites per pull-in scene, lock-regime scenes, n_ms, floor of the lock-regime locked fraction, channel-ms floor).
# The lock-regime lengths and floors come from the oracle alone over 20 seeds (tools/lock_scene_probe.py's question, per rate):
# locked fraction of the lock-regime channel-ms 0.60 at K = 1 (1000 ms), 0.50 at K = 3 (1200 ms), 0.54 at K = 5 and 0.41 at K = 6
# (1500 ms), 0.38 at K = 10 (2000 ms) -- about one scene in eight never locks at all, so the floors sit at about half of that.
BANKS = [
    (1, 2, 12, 10, 1009, 0.30, 30_000),
    (3, 2, 8, 10, 1209, 0.25, 30_000),
    (5, 2, 6, 8, 1509, 0.25, 30_000),
    (6, 2, 6, 8, 1509, 0.20, 30_000),
    (10, 2, 3, 4, 2009, 0.0, 20_000),
    (12, 8, 6, 0, 509, None, 20_000),
    (20, 4, 6, 0, 509, None, 10_000),
    (48, 4, 4, 0, 309, None, 4_000),
]


@pytest.mark.gpu
@pytest.mark.parametrize("k,n_pull_in,n_sats,n_lock,n_ms,lock_floor,min_n", BANKS, ids=[f"K{b[0]}" for b in BANKS])
def test_bank_against_the_oracle_at_every_rate(engine_factory, k, n_pull_in, n_sats, n_lock, n_ms, lock_floor, min_n):
    """ONE bank over several streams at rate K (channels addressed by stream x stride, the throughput kernel -- none of these rates
    has a speculative form -- in 250-ms launches, so every block is cut inside): every integer of every record equals the float64
    oracle's, with the bars of test_bench_shaped_banks_against_the_oracle.

    Lock-regime scenes only up to K = 10: the reference's loop gains go as 1 / fs, so a channel pulls in K times more slowly (~0.15 s
    per unit of K) and locks only once the 250-ms window behind that has filled.  At K = 12, 20 and 48 a lock-regime scene would have to
    run 2.5 .. 7.5 s -- 0.6 .. 3 GB of host IQ per stream and minutes of oracle time per channel -- so those banks are pull-in scenes,
    300 .. 500 ms long, which still cross a launch cut."""
    fs, n = 1_023_000 * k, 1023 * k
    eng = engine_factory(fs, n)
    t_start = time.time()
    t, n_chan = _multi_stream_survey(eng, _bank_specs(600000 + 1000 * k, n_pull_in, n_lock, n_sats), n_ms,
                                     f"every-rate bank K = {k}, {fs / 1e6:.3f} Msps", fs, n)
    frac = t["n_locked"] / max(1, t["n_lock"])
    print(f"[every-rate bank K = {k}] {t['n']} channel-ms compared ({n_chan} channels, {n_ms - 9} ms), {t['n_locked']} of {t['n_lock']} "
          f"lock-regime channel-ms with locked = 1 ({frac:.1%}), fast {t['fast']}, knife-edge {t['knife_edge'] + t['knife_edge_argmax']}, "
          f"UNEXPLAINED {t['unexplained']}, {time.time() - t_start:.0f} s")
    msg = (t["first"], t["events"], f"GYP_SURVEY_SEED={SEED_OFFSET}")
    assert t["fast"] == 0, t["fast"]
    assert t["n"] >= min_n, t["n"]
    assert t["n"] >= 0.9 * n_chan * (n_ms - 9) - t["n_after_event"]
    assert t["unexplained"] == 0, msg
    assert t["cp"] == 0 and t["off"] == 0 and t["lock"] == 0 and t["nudge_bad"] == 0, msg
    assert t["sym_locked"] == 0 and t["bad_locked"] == 0, msg
    assert t["sym_never_locked"] <= 1, msg
    assert t["mag"] <= 1e-4, (t["mag"], msg)
    assert t["knife_edge"] + t["knife_edge_argmax"] <= 2 and t["n_after_event"] <= 0.05 * t["n"], msg
    if lock_floor is not None:
        assert t["n_locked"] > 0 and frac >= lock_floor, (t["n_locked"], t["n_lock"], lock_floor)


# ------------------------------------------------------------------ 2. code phases at and beyond N
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2])
def test_code_phases_at_and_beyond_n(k):
    """The reference's DLL accumulator wraps at 2046 (tracker.py:299-301), not at N: at K = 1 int(self.phase) takes the values
    N .. 2045 as well -- np.roll shifts by more than a period -- and the record carries that integer, not its residue mod N.  At
    K = 2 the modulus is N itself.  Channels started at N - 1, N, N + 2 and 2045 on satellites planted at those lags mod N (strong
    enough to lock within the block), 400 ms on the throughput kernel: every record and the final state equal the oracle's."""
    fs, n = 1_023_000 * k, 1023 * k
    n_ms = 409
    starts = [n - 1, n, n + 2, 2045]
    rng = np.random.default_rng(4077 + k)
    ids = [int(s) for s in rng.choice(np.arange(1, 33), size=len(starts), replace=False)]
    a_n, v = 22.0, 0.4                  # a lock-regime amplitude (synth.lock_regime_scene): the 3-Hz loop is reached too
    sats = [synth.SyntheticSatellite(sat_id=sv, doppler_hz=float(rng.uniform(-4000, 4000)), code_phase=cp % n,
                                     carrier_phase=float(rng.uniform(0, 2 * np.pi)), amplitude=a_n / n,
                                     nav_bits=(rng.integers(0, 2, n_ms // 20 + 2) * 2 - 1).astype(np.int8), nav_bit_offset_ms=int(rng.integers(0, 20)))
            for sv, cp in zip(ids, starts)]
    scene = synth.SyntheticScene(fs=fs, n_ms=n_ms, sats=sats, noise_sigma=float(np.sqrt(v / n)), seed=4077 + k)
    iq = synth.render(scene)
    inits = np.zeros(len(sats), dtype=_lib.CHAN_INIT)
    for i, (s, cp) in enumerate(zip(sats, starts)):
        inits[i] = (0, s.sat_id, float(round(s.doppler_hz)), float(np.angle(np.exp(1j * (s.carrier_phase + 0.1)))), cp, 0)
    t0 = [orc.chunk_times(ms * n, n, fs)[0] for ms in range(9, n_ms)]
    eng = _engine_with_env(fs, n, GYP_NO_SPEC=1)
    try:
        bank = eng.create_bank(inits)
        rec = bank.track_block(iq[9 * n:], 1, n_ms - 9, t0)
        st = bank.state()
        bank.close()
    finally:
        eng.close()
    assert not np.any((rec["path_info"] & 3) == 1)
    chips = orc.generate_ca_codes()
    beyond = 0
    for i, rec_i in enumerate(inits):
        trk = orc.Tracker(orc.TrackingState(float(rec_i["doppler_hz"]), float(rec_i["carrier_phase"]), int(rec_i["code_phase"])),
                          orc.prn_as_complex(chips[int(rec_i["sat_id"]) - 1], n), fs, n)
        for j, ms in enumerate(range(9, n_ms)):
            st_, en = orc.chunk_times(ms * n, n, fs)
            r = trk.process_samples(iq[ms * n:(ms + 1) * n], st_, en)
            g = rec[i, j]
            where = (k, i, int(rec_i["code_phase"]), ms, trk.phase)
            assert int(g["code_phase"]) == r.code_phase_after, (where, int(g["code_phase"]), r.code_phase_after)
            assert int(g["peak_offset"]) == r.peak_offset, where
            assert int(g["pseudosymbol"]) == r.pseudosymbol, where
            assert bool(g["locked"]) == bool(r.locked), where
            beyond += r.code_phase_after >= n
        assert int(st["code_phase"][i]) == trk.s.current_prn_code_phase_shift, i
        assert abs(float(st["doppler_hz"][i]) - trk.s.current_doppler_shift) < 1e-4, i
        assert st["lost"][i] == 0
    print(f"[code phases beyond N, K = {k}] {len(inits)} channels x {n_ms - 9} ms equal to the oracle; {beyond} records with code phase >= N")
    if k == 1:
        assert beyond >= n_ms - 9                # the channels started at N + 2 and 2045 live beyond N (N .. 2045)


# ------------------------------------------------------------------ 5. full-sky acquisition at every rate
ACQ_SCENES = {1: 3, 3: 3, 4: 3, 5: 3, 6: 3, 10: 2, 12: 2, 16: 2, 20: 2, 48: 2}


@pytest.mark.gpu
@pytest.mark.parametrize("k", list(ACQ_SCENES), ids=[f"K{k}" for k in ACQ_SCENES])
def test_full_sky_acquisition_at_every_rate(engine_factory, k):
    """gyp_acquire of all 32 satellites of 6-satellite scenes (26 of them noise-only, where the cross-level near-ties and
    acq_exact_profile_kernel fire) against the oracle's 10-level search, one (scene, satellite) per oracle job: Doppler bin and code
    phase equal, strength within 1e-4.  How close the oracle's own search came to a cross-level tie is printed."""
    fs, n = 1_023_000 * k, 1023 * k
    eng = engine_factory(fs, n)
    t_start = time.time()
    seeds = [640000 + 100 * k + SEED_OFFSET + j for j in range(ACQ_SCENES[k])]
    jobs = [(fs, seed, sv) for seed in seeds for sv in range(1, 33)]
    want = {}
    gaps = []
    with mp.get_context("spawn").Pool(survey_worker.pool_size(len(jobs))) as pool:
        for seed, sv, dop, cp, strength, gap in pool.imap_unordered(survey_worker.run_full_sky_one, jobs):
            want[(seed, sv)] = (dop, cp, strength)
            gaps.append(gap)
    tot = noise = 0
    for seed in seeds:
        scene = synth.random_scene(fs, 10, 6, seed, with_nav_bits=False, max_code_phase=(2046 if n > 2046 else None))
        present = {s.sat_id for s in scene.sats}
        got = eng.acquire(synth.render(scene), 1, 10, list(range(1, 33)))
        for g in got:
            sv = int(g["sat_id"])
            dop, cp, strength = want[(seed, sv)]
            where = (k, seed, sv, sv in present, f"GYP_SURVEY_SEED={SEED_OFFSET}")
            assert int(g["doppler_hz"]) == dop, (where, int(g["doppler_hz"]), dop)
            assert int(g["code_phase"]) == cp, (where, int(g["code_phase"]), cp)
            assert abs(float(g["strength"]) - strength) <= 1e-4 * strength, (where, float(g["strength"]), strength)
            tot += 1
            noise += sv not in present
    assert tot == 32 * len(seeds)
    gaps = np.array(gaps)
    print(f"[full-sky acquisition K = {k}, {fs / 1e6:.3f} Msps] {tot} acquisitions ({noise} noise-only) equal to the oracle, strength within "
          f"1e-4; oracle searches with a cross-level strength gap below 1e-5: {int(np.sum(gaps < 1e-5))} (smallest {gaps.min():.1e}); "
          f"{time.time() - t_start:.0f} s")


def test_full_sky_worker_is_the_oracles_search():
    """survey_worker.run_full_sky_one (CPU): one satellite of the scene, the same answer as orc.acquire_satellite on it, and the
    smallest cross-level gap as the trace of the levels gives it."""
    fs, n, seed, sv = 1_023_000, 1023, 640123, 7
    got = survey_worker.run_full_sky_one((fs, seed, sv))
    scene = synth.random_scene(fs, 10, 6, seed, with_nav_bits=False)
    trace = []
    r = orc.acquire_satellite(sv, synth.render(scene), fs, n, orc.prn_as_complex(orc.generate_ca_codes()[sv - 1], n), trace=trace)
    assert got[:5] == (seed, sv, int(r.doppler_shift), int(r.prn_phase_shift), float(r.correlation_strength))
    strengths = [lv.strength for _, _, lv in trace]
    assert len(strengths) == 10
    want_gap = min(abs(s - max(strengths[:i])) / max(strengths[:i]) for i, s in enumerate(strengths) if i)
    assert got[5] == pytest.approx(want_gap, rel=1e-12)
    assert got[4] == max(strengths)


# ------------------------------------------------------------------ 6. strided, guarded layouts
def _guarded(streams, n, pad, gap=None):
    """One complex64 buffer: `pad` NaN samples, then the streams at a stride of len(stream) + gap samples (gap = n + 1 unless given;
    odd: odd streams start at odd sample offsets) with NaN in every gap and after the last stream.  Returns (buffer, stride)."""
    length = streams[0].size
    stride = length + (n + 1 if gap is None else gap)
    buf = np.full(pad + len(streams) * stride, np.complex64(complex(np.nan, np.nan)), dtype=np.complex64)
    for b, s in enumerate(streams):
        buf[pad + b * stride:pad + b * stride + length] = s
    return buf, stride


def _scene_streams(fs, n, n_streams, n_ms, seed):
    scenes = [synth.random_scene(fs, n_ms, 3, seed + b, max_code_phase=(2046 if n > 2046 else None)) for b in range(n_streams)]
    return scenes, [synth.render(s) for s in scenes]


def _dev_copy(eng, host):
    return eng.alloc(host.nbytes).upload(host)


def _differing_fields(got, want):
    """Fields of two record arrays whose bytes differ (field by field: the records' padding bytes are not part of the result)."""
    return [f for f in got.dtype.names if got[f].tobytes() != want[f].tobytes()]


@pytest.mark.gpu
@pytest.mark.parametrize("k", RATES)
def test_strided_guarded_layouts_give_the_packed_bits(engine_factory, k):
    """The header allows any stream_stride_samples; the kernels index stream x stride + ms x N, and the halo and prefetch code reads
    beyond a chip (at the last millisecond it must wrap, not run on).  Inputs laid out with NaN before, between and after odd-strided
    streams, inside one allocation: gyp_track_block_dev (3-stream bank, throughput kernel, and the speculative tracker where it exists),
    gyp_acquire_dev (4 streams: the two-lane split) and gyp_track_step_dev give exactly the packed host form's bytes, no NaN in any
    record, and the input buffer is unchanged afterwards."""
    fs, n = 1_023_000 * k, 1023 * k
    t_start = time.time()
    checked = []

    # --- tracking blocks
    n_ms = 100 if k in (2, 8, 16) else 40          # (the speculative tracker's sub-blocks want a longer block)
    scenes, streams = _scene_streams(fs, n, 3, n_ms, 650000 + k)
    inits = np.zeros(sum(len(s.sats) for s in scenes), dtype=_lib.CHAN_INIT)
    at = 0
    for b, s in enumerate(scenes):
        for sat in s.sats:
            inits[at] = (b, sat.sat_id, float(round(sat.doppler_hz)), float(sat.carrier_phase), sat.code_phase, 0)
            at += 1
    t0 = np.array([orc.chunk_times(ms * n, n, fs)[0] for ms in range(n_ms)])
    buf, stride = _guarded(streams, n, n)
    paths = [("throughput", _engine_with_env(fs, n, GYP_NO_SPEC=1), True)]
    if k in (2, 8, 16):
        paths.append(("speculative", engine_factory(fs, n), False))
    for label, eng, owned in paths:
        try:
            bank = eng.create_bank(inits)
            want = bank.track_block(np.concatenate(streams), 3, n_ms, t0)
            bank.close()
            d_iq, d_t0 = _dev_copy(eng, buf), _dev_copy(eng, t0)
            d_rec = eng.alloc(len(inits) * n_ms * _lib.TRACK_REC.itemsize)
            bank = eng.create_bank(inits)
            bank.track_block_dev(d_iq.ptr.value + n * 8, stride, n_ms, d_t0.ptr.value, d_rec.ptr.value)
            eng.sync()
            bank.close()
            got = d_rec.download(_lib.TRACK_REC, len(inits) * n_ms).reshape(len(inits), n_ms)
            after = d_iq.download(np.complex64, buf.size)
            for d in (d_iq, d_t0, d_rec):
                d.free()
        finally:
            if owned:
                eng.close()
        fast = float(np.mean((got["path_info"] & 3) == 1))
        assert (fast > 0.5) == (label == "speculative"), (label, fast)
        for f in ("peak_re", "peak_im", "strength", "discriminator", "doppler_hz", "carrier_phase", "error"):
            assert np.all(np.isfinite(got[f])), (label, f)
        assert not _differing_fields(got, want), (label, _differing_fields(got, want))
        assert after.tobytes() == buf.tobytes(), label                     # nothing writes into the input, padding included
        checked.append(f"track_block {label}")

    eng = engine_factory(fs, n)
    # --- one tracking millisecond at the first, a middle and the last millisecond of each stream
    chans = np.zeros(len(inits), dtype=_lib.CHAN_IN)
    for i, r in enumerate(inits):
        chans[i] = (r["stream"], r["sat_id"], r["doppler_hz"], r["carrier_phase"], r["code_phase"], 0)
    d_iq, d_ch = _dev_copy(eng, buf), _dev_copy(eng, chans)
    d_out = eng.alloc(len(chans) * _lib.CHAN_OUT.itemsize)
    for ms in (0, n_ms // 2, n_ms - 1):
        starts = np.full(3, t0[ms])
        want, _ = eng.track_step(np.concatenate([s[ms * n:(ms + 1) * n] for s in streams]), 3, starts, chans)
        d_t = _dev_copy(eng, starts)
        eng._check(eng.lib.gyp_track_step_dev(eng.ctx, C.c_void_p(d_iq.ptr.value + (n + ms * n) * 8), stride, d_t.ptr, d_ch.ptr,
                                              len(chans), d_out.ptr, None))
        eng.sync()
        got = d_out.download(_lib.CHAN_OUT, len(chans))
        d_t.free()
        for f in ("peak_re", "peak_im", "early64_re", "late64_im", "sum"):
            assert np.all(np.isfinite(got[f])), (ms, f)
        assert not _differing_fields(got, want), (ms, _differing_fields(got, want))
    assert d_iq.download(np.complex64, buf.size).tobytes() == buf.tobytes()
    for d in (d_iq, d_ch, d_out):
        d.free()
    checked.append("track_step")

    # --- the acquisition search, 4 streams (two lanes)
    _, streams = _scene_streams(fs, n, 4, 10, 660000 + k)
    buf, stride = _guarded(streams, n, n)
    ids = list(range(1, 33))
    want = eng.acquire(np.concatenate(streams), 4, 10, ids)
    d_iq = _dev_copy(eng, buf)
    d_out = eng.alloc(4 * len(ids) * _lib.ACQ_RESULT.itemsize)
    eng.acquire_dev(d_iq.ptr.value + n * 8, 4, stride, 10, ids, d_out.ptr.value)
    eng.sync()
    got = d_out.download(_lib.ACQ_RESULT, 4 * len(ids))
    assert np.all(np.isfinite(got["strength"])) and np.all(np.isfinite(got["carrier_phase"]))
    assert not _differing_fields(got, want), _differing_fields(got, want)
    assert d_iq.download(np.complex64, buf.size).tobytes() == buf.tobytes()
    d_iq.free()
    d_out.free()
    checked.append("acquire (4 streams)")
    print(f"[guarded layouts K = {k}] bit-identical to the packed form: {', '.join(checked)}; {time.time() - t_start:.1f} s")
