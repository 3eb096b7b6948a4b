#!/usr/bin/env python3
"""Device time of the weak-signal measurement on the GPU box: gyp_weak_measure_dev (the defaults: two passes, d = 1/2 chip) for 3
candidates over 220 ms and for 32 candidates over 2000 ms of one stream, at 2.046 and at 16.368 Msps; beside it, in the same run and
on the same samples, gyp_weak_refine_dev for the same candidates and a weak bank taking them through the same milliseconds in SYNC
(sync_ms = 2000: gyp_weak_track_block_dev, every call on a fresh bank).  HIP events (gyp_timer_start / gyp_timer_stop) on the
library's stream around one call, median of 5 after a warm-up.  The measure and refine calls' times hold their upload of the
candidates and the one wait behind it.  The text of profiles/weak_measure_kernels.txt.

    python tools/weak_measure_probe.py

The samples are synthetic baseband made on the device (gyp_synth_iq_dev: the candidates' satellites at 30-45 dB-Hz, Dopplers within
+-300 Hz as in tools/weak_refine_probe.py, integer code phases); every candidate starts at its satellite's Doppler and bit edge.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from gypsum_amd import _lib, _records  # noqa: E402
from gypsum_amd.engine import GypsumEngine  # noqa: E402

SIGMA = 0.05
SHAPES = ((3, 220), (32, 2000))
REPS = 5
CN0 = (30.0, 33.0, 38.0, 45.0)


def timed(eng: GypsumEngine, call) -> float:
    eng.timer_start()
    call()
    return eng.timer_stop()


def stats(times) -> str:
    return f"min {min(times):9.3f} ms   median {float(np.median(times)):9.3f} ms   max {max(times):9.3f} ms"


def run(eng: GypsumEngine, fs: int, n: int, n_cand: int, n_ms: int) -> None:
    stride = n_ms * n
    d_iq = eng.alloc(stride * 8)
    rng = np.random.default_rng(11)
    sats = np.zeros((1, n_cand), dtype=_lib.SYNTH_SAT)
    results = np.zeros(n_cand, dtype=_lib.WEAK_RESULT)
    refined = np.zeros(n_cand, dtype=_lib.WEAK_REFINED)
    ids = list(range(1, n_cand + 1)) if n_cand > 3 else [7, 19, 26]
    for i, sv in enumerate(ids):
        d, cp, phi, off = float(rng.uniform(-300, 300)), int(rng.integers(0, n)), float(rng.uniform(-np.pi, np.pi)), int(rng.integers(0, 20))
        sats[0, i] = (sv, cp, d, phi, SIGMA * np.sqrt(2.0 * 10.0 ** (CN0[i % 4] / 10.0) / (1000.0 * n)), off)
        for rec in (results, refined):
            rec[i]["sat_id"], rec[i]["doppler_hz"], rec[i]["carrier_phase"], rec[i]["code_phase"] = sv, d, phi, cp
        refined[i]["edge"] = (-off) % 20
    eng.synth_iq(d_iq, 1, stride, n_ms, sats, SIGMA, 322)
    inits = np.zeros(n_cand, dtype=_lib.CHAN_INIT)
    for name in ("stream", "sat_id", "doppler_hz", "carrier_phase", "code_phase"):
        inits[name] = results[name]
    d_out = eng.alloc(n_cand * _lib.WEAK_MEASURED.itemsize)
    d_ref = eng.alloc(n_cand * _lib.WEAK_REFINED.itemsize)
    d_ms = eng.alloc(n_cand * n_ms * _lib.WEAK_MS_REC.itemsize)

    def measure():
        eng.measure_weak_dev(d_iq.ptr.value, 1, stride, 0, n_ms, refined, d_out.ptr.value)

    def refine():
        eng.refine_weak_dev(d_iq.ptr.value, 1, stride, 0, n_ms, results, d_ref.ptr.value)

    def bank_sync() -> float:
        bank = eng.create_weak_bank(inits, _records.WeakParams(sync_ms=2000), 0)
        t = timed(eng, lambda: bank.track_block_dev(d_iq.ptr.value, stride, 0, n_ms, d_ms.ptr.value))
        bank.close()
        return t

    timed(eng, measure)
    t_measure = [timed(eng, measure) for _ in range(REPS)]
    rec = d_out.download(_lib.WEAK_MEASURED, n_cand)
    timed(eng, refine)
    t_refine = [timed(eng, refine) for _ in range(REPS)]
    bank_sync()
    t_bank = [bank_sync() for _ in range(REPS)]
    passes = 2
    print(f"{n_cand} candidates x {n_ms} ms at {fs / 1e6:.3f} Msps ({eng.device_name()}), {REPS} calls after a warm-up")
    print(f"    gyp_weak_measure_dev, {passes} passes          {stats(t_measure)}   "
          f"({passes * n_cand * n_ms * n / float(np.median(t_measure)) / 1e6:.1f} G candidate-samples/s over the passes)")
    print(f"    gyp_weak_refine_dev                    {stats(t_refine)}")
    print(f"    gyp_weak_track_block_dev, all in SYNC  {stats(t_bank)}")
    print(f"    algorithmic bytes: {stride * 8 / 1e6:.1f} MB of samples read once per pass ({passes * n_cand * stride * 8 / 1e6:.1f} MB if every candidate fetched "
          f"its own), {n_cand * n_ms * 40 / 1e3:.1f} kB of sums and W_m written per pass; {n_cand * ((n_ms + 3) // 4)} workgroups of 4 wavefronts in the sums kernel")
    err = rec["cn0_dbhz"] - np.array([CN0[i % 4] for i in range(n_cand)])
    print(f"    measured: |dd_last| median {float(np.median(np.abs(rec['dd_last']))):.4f} chip, largest {float(np.abs(rec['dd_last']).max()):.4f}; "
          f"C/N0 error median {float(np.median(np.abs(err))):.2f} dB, largest {float(np.abs(err).max()):.2f}; status 0 on {int(np.sum(rec['status'] == 0))} of {n_cand}")
    for b in (d_iq, d_out, d_ref, d_ms):
        b.free()


def main() -> None:
    for fs in (2_046_000, 16_368_000):
        eng = GypsumEngine(0)
        eng.set_stream_format(fs, fs // 1000)
        for n_cand, n_ms in SHAPES:
            run(eng, fs, fs // 1000, n_cand, n_ms)
        eng.close()


if __name__ == "__main__":
    main()
