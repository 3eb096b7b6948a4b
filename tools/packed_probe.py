#!/usr/bin/env python3
"""Packed-recording throughput on the GPU box, each case timed beside its byte-wide twin in the same run (128 streams x 250 ms,
gyp_timer_*, median of repeated launches):
  - unpack: 2-bit I,Q at 8.184 Msps (gyp_unpack_iq_dev) against the int8 widen kernel (gyp_widen_iq_dev) on the same samples;
  - down-converter 38.192 Msps at IF 9.548 MHz -> 8.184 Msps: 2-bit real (gyp_resample_packed_dev) against int8 and int16 words;
  - ingest from page cache to device blocks: a 2-bit I,Q file (gyp_ingest_open_packed) against its int8 twin (gyp_ingest_open),
    read twice, the second pass timed (wall clock from opening the handle to the last block's sync).
Prints one JSON object."""
from __future__ import annotations

import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gypsum_amd import _lib  # noqa: E402
from gypsum_amd import packing as pk  # noqa: E402
from gypsum_amd.engine import GypsumEngine  # noqa: E402
from gypsum_amd.ingest import IqFileIngest  # noqa: E402

STREAMS, N_MS, REPS = 128, 250, int(os.environ.get("GYP_PROBE_REPS", "10"))


def timed(eng, call) -> tuple[float, float]:
    call()
    eng.sync()
    times = []
    for _ in range(REPS):
        eng.timer_start()
        call()
        times.append(eng.timer_stop())
    return float(np.median(times)), float(min(times))


def upload_rows(eng, row: np.ndarray, n: int):
    d = eng.alloc(n * row.nbytes)
    for s in range(n):
        eng._check(eng.lib.gyp_memcpy_h2d(eng.ctx, _lib.C.c_void_p(d.ptr.value + s * row.nbytes), _lib.ptr(row), row.nbytes))
    eng.sync()
    return d


def main() -> None:
    eng = GypsumEngine(0)
    out = {"device": eng.device_name(), "streams": STREAMS, "ms_per_stream": N_MS, "reps": REPS, "runs": []}
    rng = np.random.default_rng(7)

    def record(d):
        out["runs"].append(d)
        print(json.dumps(d), file=sys.stderr, flush=True)

    # unpack vs widen at 8.184 Msps
    fs = 8_184_000
    eng.set_stream_format(fs, fs // 1000)
    p = pk.sign_magnitude(2)
    n = N_MS * fs // 1000
    codes = rng.integers(0, 4, 2 * n)
    packed = np.frombuffer(pk.pack(codes, p), dtype=np.uint8)
    twin = np.asarray(p.levels).astype(np.int8)[codes]
    d_p, d_t = upload_rows(eng, packed, STREAMS), upload_rows(eng, twin, STREAMS)
    d_out = eng.alloc(STREAMS * n * 8)
    ms_p = timed(eng, lambda: eng.unpack_iq_dev(p, d_p.ptr.value, STREAMS, packed.nbytes, 0, n, 0.03, n, d_out.ptr.value))
    ms_t = timed(eng, lambda: eng.widen_iq_dev(_lib.GYP_FMT_I8, d_t.ptr.value, STREAMS * twin.size, d_out.ptr.value, 0.03))
    record({"case": "unpack 2-bit IQ 8.184 Msps vs int8 widen", "packed_ms": round(ms_p[0], 4), "int8_ms": round(ms_t[0], 4),
            "ratio": round(ms_p[0] / ms_t[0], 3), "out_gsamples_per_s": round(STREAMS * n / ms_p[0] / 1e6, 2),
            "out_tb_per_s": round(STREAMS * n * 8 / ms_p[0] / 1e9, 3)})
    for b in (d_p, d_t, d_out):
        b.free()

    # down-converter 38.192 @ 9.548 -> 8.184: 2-bit real vs int8 / int16
    fs_in, if_hz = 38_192_000, 9_548_000
    n_in = N_MS * fs_in // 1000
    p = pk.sign_magnitude(2, real=True)
    codes = rng.integers(0, 4, n_in)
    packed = np.frombuffer(pk.pack(codes, p), dtype=np.uint8)
    i8 = np.asarray(p.levels).astype(np.int8)[codes]
    i16 = i8.astype(np.int16)
    d_out = eng.alloc(STREAMS * N_MS * (fs // 1000) * 8)
    res = {"case": "ddc 38.192 @ 9.548 -> 8.184 Msps, T auto (96)", "input_gb": {}}
    for name, words in (("packed2", packed), ("int8", i8), ("int16", i16)):
        d = upload_rows(eng, words, STREAMS)
        if name == "packed2":
            call = lambda: eng.resample_packed_dev(p, d.ptr.value, STREAMS, words.nbytes, 0, 0, n_in, 0.03, fs_in, if_hz, 0, 0, N_MS,
                                                   N_MS * (fs // 1000), d_out.ptr.value)
        else:
            fmt = _lib.GYP_FMT_I8 if name == "int8" else _lib.GYP_FMT_I16
            call = lambda: eng.ddc_iq_dev(fmt, d.ptr.value, STREAMS, n_in, 0, n_in, 0.03, fs_in, if_hz, 0, 0, N_MS, N_MS * (fs // 1000),
                                          d_out.ptr.value)
        res[f"{name}_ms"] = round(timed(eng, call)[0], 4)
        res["input_gb"][name] = round(STREAMS * words.nbytes / 1e9, 3)
        d.free()
    res["packed_vs_int8"] = round(res["packed2_ms"] / res["int8_ms"], 3)
    record(res)
    d_out.free()

    # ingest from page cache: 2-bit I,Q at 8.184 Msps vs the int8 twin, one stream, 4 s
    with tempfile.TemporaryDirectory() as tmp:
        secs = 8
        n = secs * fs
        p = pk.sign_magnitude(2)
        codes = rng.integers(0, 4, 2 * n)
        (Path(tmp) / "p.bin").write_bytes(pk.pack(codes, p))
        np.asarray(p.levels).astype(np.int8)[codes].tofile(Path(tmp) / "t.bin")
        res = {"case": f"ingest page cache -> device, 8.184 Msps, {secs} s, block 250 ms"}
        for name in ("packed2", "int8"):
            best = None
            for _ in range(2):   # the second pass reads from page cache; the clock includes opening (the reader starts there)
                t0 = time.perf_counter()
                if name == "packed2":
                    ing = IqFileIngest(Path(tmp) / "p.bin", fs, engine=eng, block_ms=250, packing=p)
                else:
                    ing = IqFileIngest(Path(tmp) / "t.bin", fs, np.int8, engine=eng, block_ms=250)
                while ing.next_device_block() is not None:
                    pass
                eng.sync()
                dt = time.perf_counter() - t0
                ing.close()
                best = dt
            res[f"{name}_s"] = round(best, 4)
            res[f"{name}_msps"] = round(n / best / 1e6, 1)
        res["file_mb"] = {"packed2": round(n * 4 / 8 / 1e6, 1), "int8": round(n * 2 / 1e6, 1)}
        record(res)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
