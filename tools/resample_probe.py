#!/usr/bin/env python3
"""Resampler throughput on the GPU box: gyp_resample_iq_dev on 128 streams x 250 ms already in HBM, timed with gyp_timer_*
(median of repeated launches).  Prints one JSON object: kernel time, output Gsamples/s, bytes moved per second (file-width
words read + complex64 written), per (rate pair, word format, LDS tile size)."""
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
CASES = [(4_000_000, 4_092_000), (20_000_000, 16_368_000)]
FORMATS = {"i16": (np.int16, _lib.GYP_FMT_I16, 1.0 / 8000), "f32": (np.float32, _lib.GYP_FMT_F32, 1.0)}
TILES = [int(t) for t in os.environ.get("GYP_PROBE_TILES", "2048,4096,8192").split(",")]


def main() -> None:
    eng = GypsumEngine(0)
    out = {"device": eng.device_name(), "streams": STREAMS, "ms_per_stream": N_MS, "reps": REPS, "runs": []}
    rng = np.random.default_rng(3)
    for fs_in, fs_out in CASES:
        eng.set_stream_format(fs_out, fs_out // 1000)
        n_in, n_out = fs_in // 1000, fs_out // 1000
        n_samples = N_MS * n_in
        for name, (dtype, fmt, scale) in FORMATS.items():
            block = (rng.standard_normal(2 * n_samples) * (8000 if dtype is np.int16 else 1)).astype(dtype)
            d_raw = eng.alloc(STREAMS * block.nbytes)
            for s in range(STREAMS):
                eng._check(eng.lib.gyp_memcpy_h2d(eng.ctx, _lib.C.c_void_p(d_raw.ptr.value + s * block.nbytes), _lib.ptr(block), block.nbytes))
            eng.sync()
            d_out = eng.alloc(STREAMS * N_MS * n_out * 8)
            for tile in TILES:
                eng.debug_set("resample_tile_samples", tile)
                call = lambda: eng.resample_iq_dev(fmt, d_raw.ptr.value, STREAMS, n_samples, 0, n_samples, scale, fs_in, 32, 0, N_MS,
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
                out["runs"].append({"fs_in": fs_in, "fs_out": fs_out, "format": name, "tile_samples": tile, "kernel_ms": round(ms, 4),
                                    "kernel_ms_min": round(float(min(times)), 4), "out_gsamples_per_s": round(out_samples / ms / 1e6, 2),
                                    "in_gsamples_per_s": round(STREAMS * n_samples / ms / 1e6, 2),
                                    "bytes_per_s_tb": round(moved / ms / 1e9, 3)})
                print(json.dumps(out["runs"][-1]), file=sys.stderr, flush=True)
            eng.debug_set("resample_tile_samples", 4096)
            d_raw.free()
            d_out.free()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
