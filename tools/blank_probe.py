#!/usr/bin/env python3
"""Kernel times of the pulse blanker and of its power histogram on the GPU box beside a device-to-device copy of the same samples in
the same run: the text of profiles/blank_kernels.txt (written there, or to the path given as the only argument, and to stdout).

128 streams x 100 ms at 8.184 Msps of resident complex64 samples (838 MB: beyond the Infinity Cache), noise with bursts of 41
samples every 409 at +20 dB.  The blanker at 0 % (a threshold nothing reaches), about 10 % (threshold 4 sigma, guard 4) and 100 %
(a threshold everything reaches) blanked, out of place and in place.  An in-place launch changes its input -- a second launch over
the same buffer would find the pulses gone -- so every in-place launch is timed together with the copy that restores the buffer in
front of it, and the copy's own time is subtracted.  HIP events (gyp_timer_start / gyp_timer_stop) on the library's stream around
LAUNCHES back-to-back launches, per launch; REPS repetitions after a warm-up.  A record, not a gate."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import blank_model as model  # noqa: E402
from gypsum_amd.blanker import Blanker  # noqa: E402
from gypsum_amd.engine import GypsumEngine  # noqa: E402

N_STREAMS, N_MS, N = 128, 100, 8184
LAUNCHES, REPS = 10, 5
OUT = []


def say(text: str = "") -> None:
    print(text)
    OUT.append(text)


def timed(eng, call):
    call()
    eng.sync()
    times = []
    for _ in range(REPS):
        eng.timer_start()
        for _ in range(LAUNCHES):
            call()
        times.append(eng.timer_stop() * 1e3 / LAUNCHES)       # us per launch
    return min(times), float(np.median(times)), max(times)


def line(name, t, mb, less=0.0):
    lo, med, hi = (v - less for v in t)
    say(f"{name}\n    min {lo:8.1f} us   median {med:8.1f} us   max {hi:8.1f} us   {mb:.1f} MB   {mb * 1e6 / (med * 1e-6) / 1e9:.0f} GB/s at the median")
    return med


def main() -> None:
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "blank_kernels.txt"
    eng = GypsumEngine(0)
    eng.set_stream_format(N * 1000, N)
    rng = np.random.default_rng(8184)
    count = N_MS * N
    row = (rng.standard_normal(count) + 1j * rng.standard_normal(count) + model.pulses(count, 1.0, 41, db=20.0)).astype(np.complex64)
    rows = np.ascontiguousarray(np.broadcast_to(row, (N_STREAMS, count)))
    mb = rows.nbytes / 1e6
    d_src, d_work = eng.alloc(rows.nbytes).upload(rows), eng.alloc(rows.nbytes)
    d_counts, d_hist = eng.alloc(4 * N_STREAMS * N_MS), eng.alloc(4 * model.BINS * N_STREAMS)
    p_src, p_work = d_src.ptr.value, d_work.ptr.value
    del rows
    say(f"{N_STREAMS} streams x {N_MS} ms x {N} complex64 samples in HBM ({mb:.1f} MB) on ({eng.device_name()}).")
    say(f"HIP events (gyp_timer_start / gyp_timer_stop) around {LAUNCHES} back-to-back launches, per launch; {REPS} repetitions after a warm-up.")
    say("MB and GB/s count the samples once (what the copy reads).  In-place lines: the launch together with the copy that restores the")
    say("buffer, minus the copy's median.  All lines were timed in this one run.  A record, not a gate.\n")

    def copy():
        eng.allgather_dev(p_src, p_work, count * N_STREAMS * 8)

    t_copy = timed(eng, copy)
    med_copy = line("device-to-device copy of the samples (hipMemcpyAsync on the library's stream)", t_copy, mb)
    meds = {}
    cases = (("0 % blanked", Blanker(0.0, 0.0, 1e6, 4)), ("about 10 % blanked", Blanker(0.0, 0.0, 4.0, 4)), ("100 % blanked", Blanker(0.0, 0.0, 1e-6, 4)))
    for name, b in cases:
        meds[(name, "out of place")] = line(f"iq_blank_kernel, {name}, out of place (gyp_blank_iq_dev)",
                                            timed(eng, lambda: eng.blank_iq_dev(p_src, p_work, N_STREAMS, count, N_MS, N, b, d_counts.ptr.value)), mb)
        share = d_counts.download(np.int32, N_STREAMS * N_MS).sum() / float(count * N_STREAMS)

        def in_place():
            copy()
            eng.blank_iq_dev(p_work, p_work, N_STREAMS, count, N_MS, N, b, d_counts.ptr.value)

        meds[(name, "in place")] = line(f"iq_blank_kernel, {name} (measured share {share:.4f}), in place, the restoring copy subtracted",
                                        timed(eng, in_place), mb, less=med_copy)
    meds[("histogram", "")] = line("iq_power_hist_kernel (gyp_iq_power_hist_dev, the zeroing of the histograms included)",
                                   timed(eng, lambda: eng.power_hist_dev(p_src, N_STREAMS, count, count, None, d_hist.ptr.value)), mb)
    say()
    for (name, how), med in meds.items():
        say(f"ratio to the copy, {name}{', ' if how else ''}{how}: {med / med_copy:.2f}")
    got = d_hist.download(np.uint32, model.BINS * N_STREAMS).reshape(N_STREAMS, model.BINS)
    want = model.hist(row)
    say(f"\ncheck: the histograms of streams 0 and {N_STREAMS - 1} equal the model's integers: {np.array_equal(got[0], want) and np.array_equal(got[-1], want)}")
    for d in (d_src, d_work, d_counts, d_hist):
        d.free()
    eng.close()
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
