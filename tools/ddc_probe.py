#!/usr/bin/env python3
"""Down-converter throughput on the GPU box: gyp_ddc_iq_dev on 128 streams x 250 ms of real words already in HBM, timed with
gyp_timer_* (median of repeated launches).  Prints one JSON object: kernel time, output Gsamples/s and bytes moved per second
(file-width words read + complex64 written), for 16.368 Msps int8 at IF 4.092 MHz -> 4.092 Msps (T = 64) and 38.192 Msps int16
at IF 9.548 MHz -> 8.184 Msps (T automatic: 96)."""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gypsum_amd import _lib  # noqa: E402
from gypsum_amd.engine import GypsumEngine  # noqa: E402

STREAMS, N_MS, REPS = 128, 250, int(os.environ.get("GYP_PROBE_REPS", "10"))
# (fs_in, if_hz, fs_out, taps, word type, format, scale)
CASES = [(16_368_000, 4_092_000, 4_092_000, 64, np.int8, _lib.GYP_FMT_I8, 1.0 / 60),
         (38_192_000, 9_548_000, 8_184_000, 0, np.int16, _lib.GYP_FMT_I16, 1.0 / 8000)]


def main() -> None:
    eng = GypsumEngine(0)
    out = {"device": eng.device_name(), "streams": STREAMS, "ms_per_stream": N_MS, "reps": REPS, "runs": []}
    rng = np.random.default_rng(3)
    for fs_in, if_hz, fs_out, taps, dtype, fmt, scale in CASES:
        eng.set_stream_format(fs_out, fs_out // 1000)
        n_in, n_out = fs_in // 1000, fs_out // 1000
        n_samples = N_MS * n_in
        block = np.clip(rng.standard_normal(n_samples) * (40 if dtype is np.int8 else 8000), np.iinfo(dtype).min,
                        np.iinfo(dtype).max).astype(dtype)
        d_raw = eng.alloc(STREAMS * block.nbytes)
        for s in range(STREAMS):
            eng._check(eng.lib.gyp_memcpy_h2d(eng.ctx, _lib.C.c_void_p(d_raw.ptr.value + s * block.nbytes), _lib.ptr(block), block.nbytes))
        eng.sync()
        d_out = eng.alloc(STREAMS * N_MS * n_out * 8)
        call = lambda: eng.ddc_iq_dev(fmt, d_raw.ptr.value, STREAMS, n_samples, 0, n_samples, scale, fs_in, if_hz, taps, 0, N_MS,
                                      N_MS * n_out, d_out.ptr.value)
        call()   # design upload, warm-up
        eng.sync()
        times = []
        for _ in range(REPS):
            eng.timer_start()
            call()
            times.append(eng.timer_stop())
        ms = float(np.median(times))
        out_samples = STREAMS * N_MS * n_out
        moved = STREAMS * block.nbytes + out_samples * 8
        out["runs"].append({"fs_in": fs_in, "if_hz": if_hz, "fs_out": fs_out, "taps": taps or "auto", "format": np.dtype(dtype).name,
                            "kernel_ms": round(ms, 4), "kernel_ms_min": round(float(min(times)), 4),
                            "out_gsamples_per_s": round(out_samples / ms / 1e6, 2),
                            "in_gsamples_per_s": round(STREAMS * n_samples / ms / 1e6, 2), "bytes_per_s_tb": round(moved / ms / 1e9, 3),
                            "input_gb": round(STREAMS * block.nbytes / 1e9, 3)})
        print(json.dumps(out["runs"][-1]), file=sys.stderr, flush=True)
        d_raw.free()
        d_out.free()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
