#!/usr/bin/env python3
"""Device time of the weak-signal hand-over on the GPU box: gyp_weak_refine_dev for 3 candidates over 220 ms and for 32 candidates
over 2000 ms of one stream, at 2.046 and at 16.368 Msps; beside it, in the same run and on the same samples, a weak bank taking the
same candidates through the same milliseconds in SYNC (sync_ms = 2000: gyp_weak_track_block_dev, every call on a fresh bank) and
gyp_acquire_weak_dev for the same satellites on the first 220 ms (10-ms blocks, both flags, +-7 kHz, 10 Hz fine).  HIP events
(gyp_timer_start / gyp_timer_stop) on the library's stream around one call, median of 5 after a warm-up.  The refine call's time
holds its upload of the candidates and the one wait behind it.  The text of profiles/weak_refine_kernels.txt.

    python tools/weak_refine_probe.py

The samples are synthetic baseband made on the device (gyp_synth_iq_dev: the candidates' satellites at 30-45 dB-Hz, Dopplers within
+-300 Hz as in tools/weak_track_probe.py); every candidate starts 7 Hz above its satellite's Doppler.
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
SEARCH_MS = 220
SHAPES = ((3, 220), (32, 2000))
REPS = 5


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
    ids = list(range(1, n_cand + 1)) if n_cand > 3 else [7, 19, 26]
    for i, sv in enumerate(ids):
        cn0 = (30.0, 33.0, 38.0, 45.0)[i % 4]
        d, cp, phi = float(rng.uniform(-300, 300)), int(rng.integers(0, n)), float(rng.uniform(-np.pi, np.pi))
        sats[0, i] = (sv, cp, d, phi, SIGMA * np.sqrt(2.0 * 10.0 ** (cn0 / 10.0) / (1000.0 * n)), int(rng.integers(0, 20)))
        results[i]["sat_id"], results[i]["doppler_hz"], results[i]["carrier_phase"], results[i]["code_phase"] = sv, d + 7.0, phi, cp
    eng.synth_iq(d_iq, 1, stride, n_ms, sats, SIGMA, 322)
    inits = np.zeros(n_cand, dtype=_lib.CHAN_INIT)
    for name in ("stream", "sat_id", "doppler_hz", "carrier_phase", "code_phase"):
        inits[name] = results[name]
    d_out = eng.alloc(n_cand * _lib.WEAK_REFINED.itemsize)
    d_prompts = eng.alloc(n_cand * n_ms * 8)
    d_ms = eng.alloc(n_cand * n_ms * _lib.WEAK_MS_REC.itemsize)
    d_search = eng.alloc(n_cand * _lib.WEAK_RESULT.itemsize)

    def refine():
        eng.refine_weak_dev(d_iq.ptr.value, 1, stride, 0, n_ms, results, d_out.ptr.value, None, d_prompts.ptr.value)

    def bank_sync() -> float:
        bank = eng.create_weak_bank(inits, _records.WeakParams(sync_ms=2000), 0)
        t = timed(eng, lambda: bank.track_block_dev(d_iq.ptr.value, stride, 0, n_ms, d_ms.ptr.value))
        bank.close()
        return t

    def search():
        eng.acquire_weak_dev(d_iq.ptr.value, 1, stride, 10, SEARCH_MS // 10, _lib.GYP_HYB_ALTERNATE | _lib.GYP_HYB_CODE_DOPPLER, ids, 0.0, 7000.0, 10.0,
                             d_search.ptr.value)

    timed(eng, refine)
    t_refine = [timed(eng, refine) for _ in range(REPS)]
    rec = d_out.download(_lib.WEAK_REFINED, n_cand)
    bank_sync()
    t_bank = [bank_sync() for _ in range(REPS)]
    timed(eng, search)
    t_search = [timed(eng, search) for _ in range(REPS)]
    err = np.abs(rec["delta_hz"] + 7.0)
    print(f"{n_cand} candidates x {n_ms} ms at {fs / 1e6:.3f} Msps ({eng.device_name()}), {REPS} calls after a warm-up")
    print(f"    gyp_weak_refine_dev                    {stats(t_refine)}   ({n_cand * n_ms * n / float(np.median(t_refine)) / 1e6:.1f} G candidate-samples/s)")
    print(f"    gyp_weak_track_block_dev, all in SYNC  {stats(t_bank)}")
    print(f"    gyp_acquire_weak_dev on {SEARCH_MS} ms           {stats(t_search)}")
    print(f"    algorithmic bytes: {stride * 8 / 1e6:.1f} MB of samples read once ({n_cand * stride * 8 / 1e6:.1f} MB if every candidate fetched its own), "
          f"{n_cand * n_ms * 8 / 1e3:.1f} kB of prompts written; {n_cand * ((n_ms + 3) // 4)} workgroups of 4 wavefronts in the sums kernel")
    print(f"    refined: |delta_hz + 7| median {float(np.median(err)):.3f} Hz, largest {float(err.max()):.3f} Hz; status 0 on {int(np.sum(rec['status'] == 0))} of {n_cand}")
    for b in (d_iq, d_out, d_prompts, d_ms, d_search):
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
