#!/usr/bin/env python3
"""Kernel times of the excisor and of its bin-power histogram on the GPU box beside a device-to-device copy of the same samples in
the same run: the text of profiles/excise_kernels.txt (written there, or to the path given as the only argument, and to stdout).

512 streams x 100 ms at 2.046 Msps of resident complex64 samples (838 MB: beyond the Infinity Cache): the clean twin of the "fm"
scene of tests/excise_model.py, and the scene itself with its 40 dB FM jammer; the excisor is the one the device's histogram of the
jammed scene gives (factor 16, guard 1).  Out of place and in place.  An in-place launch changes its input -- a second launch over
the same buffer would find the jammer gone -- so every in-place launch is timed together with the copy that restores the buffer in
front of it, and the copy's own time is subtracted.  HIP events (gyp_timer_start / gyp_timer_stop) on the library's stream around
LAUNCHES back-to-back launches, per launch; REPS repetitions after a warm-up.  A record, not a gate."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import excise_model as model  # noqa: E402
from gypsum_amd.engine import GypsumEngine  # noqa: E402
from gypsum_amd.excisor import excisor_from_hist, n_frames  # noqa: E402

N_STREAMS, N_MS, N = 512, 100, model.SCENE_N
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
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "excise_kernels.txt"
    eng = GypsumEngine(0)
    eng.set_stream_format(model.SCENE_FS, N)
    jammed, clean = model.scene("fm", N_MS)
    count = N_MS * N
    mb = N_STREAMS * count * 8 / 1e6
    d_src, d_work = eng.alloc(N_STREAMS * count * 8), eng.alloc(N_STREAMS * count * 8)
    d_counts, d_hist = eng.alloc(4 * N_STREAMS * N_MS), eng.alloc(4 * model.BINS * N_STREAMS)
    p_src, p_work = d_src.ptr.value, d_work.ptr.value
    say(f"{N_STREAMS} streams x {N_MS} ms x {N} complex64 samples in HBM ({mb:.1f} MB) on ({eng.device_name()}).")
    say(f"HIP events (gyp_timer_start / gyp_timer_stop) around {LAUNCHES} back-to-back launches, per launch; {REPS} repetitions after a warm-up.")
    say("MB and GB/s count the samples once (what the copy reads).  In-place lines: the launch together with the copy that restores the")
    say("buffer, minus the copy's median.  All lines were timed in this one run.  A record, not a gate.\n")

    def copy():
        eng.allgather_dev(p_src, p_work, count * N_STREAMS * 8)

    e, measured = excisor_from_hist(eng.spectrum_hist(jammed[:10 * N], N), 16.0, 1)
    say(f"excisor from the jammed scene's first 10 ms: {e}, {measured}\n")
    meds = {}
    med_copy = None
    for name, row in (("clean", clean), ("fm", jammed)):
        d_src.upload(np.ascontiguousarray(np.broadcast_to(row, (N_STREAMS, count))))
        if med_copy is None:
            med_copy = line("device-to-device copy of the samples (hipMemcpyAsync on the library's stream)", timed(eng, copy), mb)
        meds[(name, "out of place")] = line(f"iq_excise_kernel, {name} buffer, out of place (gyp_excise_iq_dev, counts, no masks)",
                                            timed(eng, lambda: eng.excise_iq_dev(p_src, p_work, N_STREAMS, count, N_MS, N, e, d_counts.ptr.value)), mb)
        share = d_counts.download(np.int32, N_STREAMS * N_MS).sum() / float(256 * n_frames(N) * N_MS * N_STREAMS)

        def in_place():
            copy()
            eng.excise_iq_dev(p_work, p_work, N_STREAMS, count, N_MS, N, e, d_counts.ptr.value)

        meds[(name, "in place")] = line(f"iq_excise_kernel, {name} buffer (excised share of (frame, bin) cells {share:.4f}), in place, the restoring copy subtracted",
                                        timed(eng, in_place), mb, less=med_copy)
        meds[(name, "histogram")] = line(f"iq_spectrum_hist_kernel, {name} buffer (gyp_iq_spectrum_hist_dev, the zeroing of the histograms included)",
                                         timed(eng, lambda: eng.spectrum_hist_dev(p_src, N_STREAMS, count, N_MS, N, d_hist.ptr.value)), mb)
    # the persistent grid holds 2 workgroups per CU (8 wavefronts); the same launch on 8 per CU says what more wavefronts would hide
    try:
        eng.debug_set("widen_wg_per_cu", 8)
        meds[("fm", "out of place at 8 workgroups per CU (gyp_debug_set widen_wg_per_cu)")] = line(
            "iq_excise_kernel, fm buffer, out of place, widen_wg_per_cu = 8",
            timed(eng, lambda: eng.excise_iq_dev(p_src, p_work, N_STREAMS, count, N_MS, N, e, d_counts.ptr.value)), mb)
        meds[("fm", "histogram at 8 workgroups per CU")] = line(
            "iq_spectrum_hist_kernel, fm buffer, widen_wg_per_cu = 8",
            timed(eng, lambda: eng.spectrum_hist_dev(p_src, N_STREAMS, count, N_MS, N, d_hist.ptr.value)), mb)
    finally:
        eng.debug_set("widen_wg_per_cu", 2)
    say()
    for (name, how), med in meds.items():
        say(f"ratio to the copy, {name} buffer, {how}: {med / med_copy:.2f}")
    got = d_hist.download(np.uint32, model.BINS * N_STREAMS).reshape(N_STREAMS, model.BINS)
    say(f"\ncheck: the histograms of streams 0 and {N_STREAMS - 1} are equal and count {256 * len(model.full_frames(N)) * N_MS} powers: "
        f"{np.array_equal(got[0], got[-1]) and int(got[0].sum()) == 256 * len(model.full_frames(N)) * N_MS}")
    for d in (d_src, d_work, d_counts, d_hist):
        d.free()
    eng.close()
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
