#!/usr/bin/env python3
"""Device time of the weak bank on the GPU box: gyp_weak_track_block_dev for 12 channels of one stream and for 1536 channels over
128 streams (12 each), 1 s at 8.184 Msps in one call, beside gyp_track_block_dev (the 1-ms bank) on the same bank shape and samples
in the same run; HIP events (gyp_timer_start / gyp_timer_stop) on the library's stream around one call, median of 5 after a warm-up,
every call on a fresh bank.  The text of profiles/weak_track_kernels.txt.

    python tools/weak_track_probe.py               the timings, both shapes
    python tools/weak_track_probe.py --small       the 12-channel shape alone
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d <dir> -o weak -- python tools/weak_track_probe.py --small --once --weak-only
                                                   the kernel's fetched bytes, to set against the algorithmic bytes printed here

The samples are synthetic baseband made on the device (gyp_synth_iq_dev: twelve satellites per stream at 30-45 dB-Hz).  That
generator renders no code Doppler, which the weak bank's carrier aiding assumes (at 4.5 kHz an aided replica walks 1.2 chips off
such a signal in the 400 ms of open loop), so the Dopplers here stay within +-300 Hz: every channel then tracks to the end of the
second and the timing holds no channel that was lost and stopped working.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from gypsum_amd import _lib  # noqa: E402
from gypsum_amd.engine import GypsumEngine  # noqa: E402

FS, N, N_MS = 8_184_000, 8184, 1000
SATS = (7, 19, 26, 3, 15, 12, 1, 9, 22, 28, 30, 5)
SIGMA = 0.05


def run(eng: GypsumEngine, n_streams: int, reps: int, weak_only: bool) -> None:
    n_chan = n_streams * len(SATS)
    stride = N_MS * N
    d_iq = eng.alloc(n_streams * stride * 8)
    sats = np.zeros((n_streams, len(SATS)), dtype=_lib.SYNTH_SAT)
    inits = np.zeros(n_chan, dtype=_lib.CHAN_INIT)
    rng = np.random.default_rng(11)
    for s in range(n_streams):
        for i, sv in enumerate(SATS):
            cn0 = (30.0, 33.0, 38.0, 45.0)[i % 4]
            d, cp, phi = float(rng.uniform(-300, 300)), int(rng.integers(0, N)), float(rng.uniform(0, 2 * np.pi))
            sats[s, i] = (sv, cp, d, phi, SIGMA * np.sqrt(2.0 * 10.0 ** (cn0 / 10.0) / (1000.0 * N)), int(rng.integers(0, 20)))
            inits[s * len(SATS) + i] = (s, sv, d + 4.0, phi, cp, 0)
    eng.synth_iq(d_iq, n_streams, stride, N_MS, sats, SIGMA, 322)
    d_ms = eng.alloc(n_chan * N_MS * _lib.WEAK_MS_REC.itemsize)
    d_per = eng.alloc(n_chan * (N_MS // 20 + 1) * _lib.WEAK_PERIOD_REC.itemsize)
    d_cnt = eng.alloc(n_chan * 4)
    d_rec = eng.alloc(n_chan * N_MS * _lib.TRACK_REC.itemsize)
    d_t0 = eng.alloc(N_MS * 8).upload(np.arange(N_MS, dtype=np.float64) * 1e-3)

    def weak():
        bank = eng.create_weak_bank(inits, None, 0)
        eng.timer_start()
        bank.track_block_dev(d_iq.ptr.value, stride, 0, N_MS, d_ms.ptr.value, d_per.ptr.value, d_cnt.ptr.value)
        t = eng.timer_stop()
        st = bank.state()
        bank.close()
        return t, st

    def plain():
        bank = eng.create_bank(inits)
        eng.timer_start()
        bank.track_block_dev(d_iq.ptr.value, stride, N_MS, d_t0.ptr.value, d_rec.ptr.value)
        t = eng.timer_stop()
        del bank
        return t

    weak()
    tw = [weak() for _ in range(reps)]
    st = tw[-1][1]
    tw = [t for t, _ in tw]
    print(f"{n_chan} channels over {n_streams} stream(s), {N_MS} ms at {FS / 1e6:.3f} Msps in one call ({eng.device_name()}), {reps} call(s) after a warm-up")
    print(f"    gyp_weak_track_block_dev  min {min(tw):9.2f} ms   median {float(np.median(tw)):9.2f} ms   max {max(tw):9.2f} ms   "
          f"({n_chan * N_MS * N / float(np.median(tw)) / 1e6:.1f} G channel-samples/s)")
    if not weak_only:
        plain()
        tp = [plain() for _ in range(reps)]
        print(f"    gyp_track_block_dev       min {min(tp):9.2f} ms   median {float(np.median(tp)):9.2f} ms   max {max(tp):9.2f} ms")
    print(f"    algorithmic bytes: {n_streams * stride * 8 / 1e9:.3f} GB of samples read once per stream ({n_chan * stride * 8 / 1e9:.3f} GB if every channel "
          f"fetched its own), {n_chan * N_MS * 32 / 1e6:.1f} MB of millisecond records written")
    print(f"    after the second: {int(np.sum(st['phase'] == 2))} channels in TRACK, {int(np.sum(st['status'] == 2))} lost, "
          f"periods per channel {int(st['n_periods'].min())}..{int(st['n_periods'].max())}")
    for b in (d_iq, d_ms, d_per, d_cnt, d_rec, d_t0):
        b.free()


def main() -> None:
    reps = 1 if "--once" in sys.argv else 5
    eng = GypsumEngine(0)
    eng.set_stream_format(FS, N)
    for n_streams in (1,) if "--small" in sys.argv else (1, 128):
        run(eng, n_streams, reps, "--weak-only" in sys.argv)
    eng.close()


if __name__ == "__main__":
    main()
