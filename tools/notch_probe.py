#!/usr/bin/env python3
"""Kernel times of the notch on the GPU box, beside the condition kernel on the same block in the same run, and the suppression
the notch reaches on the end-to-end scene: the text of profiles/notch_kernels.txt on stdout.

One block of 250 ms at 8.184 Msps in HBM; HIP events (gyp_timer_start / gyp_timer_stop) around LAUNCHES back-to-back launches, per
launch; REPS repetitions after a warm-up.  The scan is the default one of gyp_ingest_find_tones over 10 ms of the same block."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import notch_model as model  # noqa: E402
from gypsum_amd.engine import GypsumEngine  # noqa: E402
from gypsum_amd.level import IqLevel  # noqa: E402

FS, N, N_MS = 8_184_000, 8184, 250
LAUNCHES, REPS = 50, 7
TONES = [217_300, -1_403_000, 2_650_000, -3_015_000]


def timed(eng, call, launches=LAUNCHES):
    call()
    eng.sync()
    times = []
    for _ in range(REPS):
        eng.timer_start()
        for _ in range(launches):
            call()
        times.append(eng.timer_stop() * 1e3 / launches)       # us per launch
    return min(times), float(np.median(times)), max(times)


def line(name, t, moved_mb=None):
    lo, med, hi = t
    rate = f"   {moved_mb:.1f} MB moved   {moved_mb * 1e6 / (med * 1e-6) / 1e9:.0f} GB/s at the median" if moved_mb else ""
    print(f"{name}\n    min {lo:8.1f} us   median {med:8.1f} us   max {hi:8.1f} us{rate}")


def main() -> None:
    eng = GypsumEngine(0)
    eng.set_stream_format(FS, N)
    count = N_MS * N
    rng = np.random.default_rng(8184)
    x = (0.05 * (rng.standard_normal(count) + 1j * rng.standard_normal(count))).astype(np.complex128)
    for k, f in enumerate(TONES):
        x += (5.0 / (k + 1)) * model.mixer(f, 0, count, FS)
    x = x.astype(np.complex64)
    d_in, d_out = eng.alloc(x.nbytes).upload(x), eng.alloc(x.nbytes)
    mb = x.nbytes / 1e6
    print(f"One block of {N_MS} ms at {FS / 1e6:.3f} Msps ({count} complex64 samples, {mb:.1f} MB) on ({eng.device_name()}).")
    print(f"HIP events (gyp_timer_start / gyp_timer_stop) around {LAUNCHES} back-to-back launches, per launch; {REPS} repetitions after a warm-up.")
    print("Bytes are what the kernel must read and write from and to memory once (the LDS form keeps the residual on the CU; the form")
    print("without LDS re-reads and re-writes it per tone, from L2 where it fits); the block fits the 256 MiB Infinity Cache, so the")
    print("rates are not HBM rates.  All kernels were timed in this one run.  The numbers are a record, not a gate.\n")
    level = IqLevel(0.01, -0.02, 0.5)
    p_in, p_out = d_in.ptr.value, d_out.ptr.value
    line("iq_condition_kernel (gyp_condition_iq_dev, out of place)", timed(eng, lambda: eng.condition_iq_dev(p_in, p_out, 1, count, count, level)), 2 * mb)
    line("iq_condition_kernel (gyp_condition_iq_dev, in place)", timed(eng, lambda: eng.condition_iq_dev(p_out, p_out, 1, count, count, level)), 2 * mb)
    for k in (1, 4):
        for no_lds in (0, 1):
            eng.debug_set("notch_no_lds", no_lds)
            form = "residual in the output buffer (notch_no_lds)" if no_lds else "residual in LDS"
            line(f"iq_notch_kernel K = {k}, {form} (gyp_notch_iq_dev, out of place)",
                 timed(eng, lambda: eng.notch_iq_dev(p_in, p_out, 1, count, 0, N_MS, N, FS, [TONES[:k]])), 2 * mb)
            line(f"iq_notch_kernel K = {k}, {form} (gyp_notch_iq_dev, in place, as on an ingest handle)",
                 timed(eng, lambda: eng.notch_iq_dev(p_out, p_out, 1, count, 0, N_MS, N, FS, [TONES[:k]])), 2 * mb)
    eng.debug_set("notch_no_lds", 0)
    grid = [(1 if k >= 0 else -1) * ((abs(k) * FS + 1024) // 2048) for k in range(-921, 922)]
    n_blocks = 10 * N // 1024
    d_rec = eng.alloc(n_blocks * len(grid) * 16)
    line(f"iq_tones_kernel, the default scan over 10 ms: {len(grid)} frequencies x {n_blocks} Hann blocks of 1024 samples = "
         f"{len(grid) * n_blocks * 1024 / 1e6:.0f} M mixer evaluations\n(gyp_iq_tones_dev, one call per repetition, the 15 KB upload of the frequency list included)",
         timed(eng, lambda: eng.iq_tones_dev(p_in, 1, count, 0, n_blocks, 1024, FS, grid, model.HANN, d_rec.ptr.value), launches=1))
    got = d_out.download(np.complex64, count)
    left = np.abs(model.tones(got[:N], FS, TONES, N, model.RECT, 0))[0]
    print(f"\ncheck: |A| of the four tones in the first millisecond of the last notched block {', '.join(f'{v:.2e}' for v in left)} (planted 5, 2.5, 1.67, 1.25)")
    for d in (d_in, d_out, d_rec):
        d.free()
    # suppression on the end-to-end scene (2.046 Msps, 10 ms, a CW 40 dB above sigma at +217 300 Hz): tests/test_gpu_notch.py's figures
    print("\nSuppression: residual power in +-500 Hz around the tone (float64 DFT of the whole 10 ms on a 25 Hz grid), before / after,")
    print("on the scene of tests/notch_model.py; the test asserts device within 1 dB of the model.")
    eng2 = GypsumEngine(0)
    eng2.set_stream_format(model.SCENE_FS, model.SCENE_N)
    for off in (0.0, 0.4, 50.0):
        s, _ = model.scene(10, tone_offset_hz=off)
        dev = eng2.notch_iq(s, model.SCENE_FS, model.SCENE_N, [model.SCENE_TONE_HZ])
        ref, _ = model.notch(s, model.SCENE_FS, model.SCENE_N, [model.SCENE_TONE_HZ])
        b, a_dev, a_ref = (model.band_power(v, model.SCENE_FS, model.SCENE_TONE_HZ + off) for v in (s, dev, ref))
        print(f"    tone {off:4.1f} Hz off its listed frequency: device {10 * np.log10(b / a_dev):6.2f} dB   float64 model {10 * np.log10(b / a_ref):6.2f} dB")
    eng2.close()
    eng.close()


if __name__ == "__main__":
    main()
