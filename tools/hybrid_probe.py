#!/usr/bin/env python3
"""Device time of the weak-signal search on the GPU box: gyp_acquire_weak_dev over 32 satellites, +-7 kHz coarse and the 10 Hz fine
level, coherent_ms = 10, both flags, 1 s of one stream (100 blocks), at 2.046 and 8.184 Msps; HIP events (gyp_timer_start /
gyp_timer_stop) on the library's stream around one call, median of 5 after a warm-up.  The text of profiles/hybrid_kernels.txt.

    python tools/hybrid_probe.py              the timings
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o hybrid -- python tools/hybrid_probe.py --once
    python tools/hybrid_probe.py --stats <dir>/.../hybrid_kernel_stats.csv     the split between the cells kernel and the new ones

The samples are synthetic baseband made on the device (gyp_synth_iq_dev: four satellites at 30-45 dB-Hz); the search's cost does
not depend on what the samples hold.
"""
from __future__ import annotations

import csv
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from gypsum_amd import _lib  # noqa: E402
from gypsum_amd.engine import GypsumEngine  # noqa: E402

T, N_MS, FLAGS = 10, 1000, _lib.GYP_HYB_ALTERNATE | _lib.GYP_HYB_CODE_DOPPLER
SPREAD, FINE = 7000.0, 10.0
RATES = ((2_046_000, 2046), (8_184_000, 8184))


def run(fs: int, n: int, reps: int) -> None:
    eng = GypsumEngine(0)
    eng.set_stream_format(fs, n)
    d_iq = eng.alloc(N_MS * n * 8)
    sats = np.zeros((1, 4), dtype=_lib.SYNTH_SAT)
    sigma = 0.05
    for i, (sv, cn0, d, cp) in enumerate(((7, 30.0, 4487.0, 0), (19, 30.0, -4462.0, n - 1), (26, 33.0, 1233.0, 700), (3, 45.0, -2871.0, 1391))):
        sats[0, i] = (sv, cp, d, 0.3 * i, sigma * np.sqrt(2.0 * 10.0 ** (cn0 / 10.0) / (1000.0 * n)), 5 * i)
    eng.synth_iq(d_iq, 1, N_MS * n, N_MS, sats, sigma, 322)
    d_out = eng.alloc(32 * _lib.WEAK_RESULT.itemsize)
    ids = list(range(1, 33))

    def call():
        eng.acquire_weak_dev(d_iq.ptr.value, 1, N_MS * n, T, N_MS // T, FLAGS, ids, 0.0, SPREAD, FINE, d_out.ptr.value)

    call()
    eng.sync()
    times = []
    for _ in range(reps):
        eng.timer_start()
        call()
        times.append(eng.timer_stop())
    res = d_out.download(_lib.WEAK_RESULT, 32)
    n_coarse, n_fine = int(2 * SPREAD / (500.0 / T)), 2 * int(250.0 / T / FINE) + 1
    cells = 32 * (n_coarse + n_fine)
    acc_bytes = cells * (N_MS // T) * n * 16 - cells * 2 * n * 4      # 8 read + 4 read + 4 written per lag and block; a set's first block reads no power
    print(f"{fs / 1e6:.3f} Msps on ({eng.device_name()}): gyp_acquire_weak_dev, 32 satellites x ({n_coarse} coarse + {n_fine} fine bins) x {N_MS // T} blocks of {T} ms, "
          f"{int(eng.debug_get('last_hybrid_chunks'))} chunk(s) in the last level")
    print(f"    device time min {min(times):9.2f} ms   median {float(np.median(times)):9.2f} ms   max {max(times):9.2f} ms   ({reps} calls after a warm-up)")
    print(f"    hybrid_accumulate_kernel traffic per call: {acc_bytes / 1e9:.2f} GB; cells kernel profile writes: {cells * (N_MS // T) * n * 8 / 1e9:.2f} GB")
    found = sorted((int(r['sat_id']), round(float(r['z']), 1), float(r['doppler_hz']), int(r['code_phase'])) for r in res if float(r['z']) > 13.4375)
    print(f"    above z = 13.4375: {found}")
    d_iq.free()
    d_out.free()
    eng.close()


def stats(path: str) -> None:
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print(f"kernel time by kernel, a warm-up and one call per rate ({path.split('/')[-1]}): total {total / 1e6:.1f} ms")
    groups = {}
    for r in rows:
        name = r["Name"]
        key = "hybrid_accumulate_kernel" if "hybrid_accumulate" in name else "hybrid_reduce_kernel" if "hybrid_reduce" in name else \
              "other hybrid_* kernels" if "hybrid_" in name else "corr_cells_kernel (coherent)" if "corr_cells" in name else "other (synthetic samples)"
        g = groups.setdefault(key, [0.0, 0])
        g[0] += float(r["TotalDurationNs"])
        g[1] += int(r["Calls"])
    for key, (ns, calls) in sorted(groups.items(), key=lambda kv: -kv[1][0]):
        print(f"    {key:34s} {ns / 1e6:10.2f} ms  {100 * ns / total:5.1f} %  {calls:7d} launches")


def main() -> None:
    if sys.argv[1:2] == ["--stats"]:
        stats(sys.argv[2])
        return
    reps = 1 if "--once" in sys.argv else 5
    for fs, n in RATES:
        run(fs, n, reps)


if __name__ == "__main__":
    main()
