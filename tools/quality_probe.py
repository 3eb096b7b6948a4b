#!/usr/bin/env python3
"""Kernel time of the signal-quality sums on the GPU box beside a device-to-device copy of the same records in the same run, and
the end-to-end C/N0 of tests/test_gpu_quality.py's scene on the device and through the float64 oracle: the text of
profiles/quality_kernels.txt on stdout.

1536 channels x 1000 ms of resident gyp_track_rec records (the headline workload's block: 86 MB), window 1000 and window 20; HIP
events (gyp_timer_start / gyp_timer_stop) on the library's stream around LAUNCHES back-to-back launches, per launch; REPS
repetitions after a warm-up."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import quality_model as model  # noqa: E402
from gypsum_amd import _lib  # noqa: E402
from gypsum_amd.engine import GypsumEngine  # noqa: E402

N_CHAN, N_MS = 1536, 1000
LAUNCHES, REPS = 50, 7


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


def line(name, t, mb):
    lo, med, hi = t
    print(f"{name}\n    min {lo:8.1f} us   median {med:8.1f} us   max {hi:8.1f} us   {mb:.1f} MB   {mb * 1e6 / (med * 1e-6) / 1e9:.0f} GB/s at the median")
    return med


def main() -> None:
    eng = GypsumEngine(0)
    eng.set_stream_format(2_046_000, 2046)
    rng = np.random.default_rng(1536)
    offs = rng.integers(0, 20, N_CHAN).astype(np.int32)
    row = model.records_from_peaks(model.synthetic_peaks(20.0, 5.1, N_MS, 0, seed=1), locked=rng.integers(0, 2, N_MS))
    recs = np.ascontiguousarray(np.broadcast_to(row, (N_CHAN, N_MS)))
    mb = recs.nbytes / 1e6
    d_rec, d_copy = eng.alloc(recs.nbytes).upload(recs), eng.alloc(recs.nbytes)
    d_out = eng.alloc(N_CHAN * (N_MS // 20) * _lib.QUALITY_SUMS.itemsize)
    p_rec, p_copy, p_out = d_rec.ptr.value, d_copy.ptr.value, d_out.ptr.value
    print(f"{N_CHAN} channels x {N_MS} ms of gyp_track_rec records in HBM ({mb:.1f} MB) on ({eng.device_name()}).")
    print(f"HIP events (gyp_timer_start / gyp_timer_stop) around {LAUNCHES} back-to-back launches, per launch; {REPS} repetitions after a warm-up.")
    print("The kernel reads 12 of each record's 56 bytes once for the moments and, with bit offsets, once more for the 20-ms groups; MB and")
    print("GB/s count the whole records (what the copy moves), so the kernel's rate is a figure of merit against the copy, not its traffic.")
    print("The records fit the 256 MiB Infinity Cache, so these are not HBM rates.  All lines were timed in this one run.  A record, not a gate.\n")
    copy = line("device-to-device copy of the records (hipMemcpyAsync on the library's stream: gyp_allgather_dev in a one-process world)",
                timed(eng, lambda: eng.allgather_dev(p_rec, p_copy, recs.nbytes)), mb)
    meds = {}
    for W in (1000, 20):
        for name, b in (("bit offsets 0..19 (moments and groups)", offs), ("no bit offsets (moments only)", None)):
            meds[(W, name)] = line(f"track_quality_kernel W = {W}, {name} (gyp_track_quality_dev)",
                                   timed(eng, lambda: eng.track_quality_dev(p_rec, N_CHAN, N_MS, N_MS, W, p_out, b)), mb)
    print()
    for (W, name), med in meds.items():
        print(f"ratio to the copy, W = {W}, {name}: {med / copy:.2f}")
    got = d_out.download(_lib.QUALITY_SUMS, N_CHAN * (N_MS // 20)).reshape(N_CHAN, N_MS // 20)      # the last launch: W = 20, no offsets
    want = model.track_quality(recs[:1], 20, None)[0]
    print(f"\ncheck: the last launch's sums of channels 0 and {N_CHAN - 1} equal the model's bits: {got[0].tobytes() == want.tobytes() and got[-1].tobytes() == want.tobytes()}")
    for d in (d_rec, d_copy, d_out):
        d.free()
    import test_gpu_quality as tq
    f = tq.e2e_figures(eng)
    print(f"\nEnd to end (tests/test_gpu_quality.py: one satellite at 2.046 Msps, seed {tq.E2E_SEED}, tracked {tq.E2E_MS} ms, W = 1000 from record {tq.E2E_FROM}):")
    print("    " + f["text"])
    eng.close()


if __name__ == "__main__":
    main()
