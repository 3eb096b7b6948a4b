"""`GypsumEngine`: thin Python object over one libgypsum_hip context (one per GPU).

All numerics happen in the HIP library; this module only marshals numpy arrays
through ctypes.  Nothing here computes a correlation on the CPU, and construction
fails if the library or a gfx950 device is missing.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import (ACQ_RESULT, CELL, CELL_DESC, CHAN_IN, CHAN_INIT, CHAN_OUT, GYP_COHERENT, GYP_NON_COHERENT, PARAMS,
                   SYNTH_SAT, TRACK_REC, GypsumHipError, ptr)


def _as_iq(iq: np.ndarray) -> np.ndarray:
    """complex64, C-contiguous view/copy of the caller's samples (the reference hands complex64 chunks)."""
    return np.ascontiguousarray(iq, dtype=np.complex64)


def _iq_arg(iq: np.ndarray, factors: Sequence[int], check: bool = True) -> np.ndarray:
    """The samples of a host form, flat complex64: as many as the product of `factors` (streams, milliseconds, samples per
    millisecond), or ValueError; check=False where the count is not one the library takes, which is then the library's to refuse."""
    iq = _as_iq(iq).reshape(-1)
    if check and iq.size != int(np.prod(factors, dtype=np.int64)):
        raise ValueError(f"expected {'*'.join(str(f) for f in factors)} samples, got {iq.size}")
    return iq


def _ids(sat_ids: Sequence[int]) -> np.ndarray:
    return np.ascontiguousarray(sat_ids, dtype=np.int32)


def _bins(doppler_hz: Sequence[float]) -> np.ndarray:
    return np.ascontiguousarray(doppler_hz, dtype=np.float64)


def hybrid_stats(cells: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """gyp_hybrid_stats (host only, no GPU): (z, peak_ratio) float64 arrays of the shape of the HYBRID_CELL records `cells`;
    z = (peak - mean_off) / std_off is NaN where it is not defined."""
    lib = _lib.load()
    c = np.ascontiguousarray(cells, dtype=_lib.HYBRID_CELL)
    flat = c.reshape(-1)
    z = np.empty(flat.size, dtype=np.float64)
    ratio = np.empty(flat.size, dtype=np.float64)
    zz, rr = C.c_double(), C.c_double()
    for i in range(flat.size):
        rc = lib.gyp_hybrid_stats(ptr(flat[i:i + 1]), C.byref(zz), C.byref(rr))
        if rc != 0:
            raise GypsumHipError(rc, (lib.gyp_last_error(None) or b"").decode())
        z[i], ratio[i] = zz.value, rr.value
    return z.reshape(c.shape), ratio.reshape(c.shape)


def hybrid_shift(n: int, coherent_ms: int, block: int, doppler_hz: float, flags: int) -> int:
    """gyp_hybrid_shift (host only, no GPU): samples by which block `block`'s peak sits earlier than block 0's."""
    return int(_lib.load().gyp_hybrid_shift(int(n), int(coherent_ms), int(block), float(doppler_hz), int(flags)))


class DeviceBuffer:
    """RAII wrapper around gyp_malloc / gyp_free."""

    def __init__(self, engine: "GypsumEngine", nbytes: int) -> None:
        self.engine = engine
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        engine._check(engine.lib.gyp_malloc(engine.ctx, max(1, self.nbytes), C.byref(p)))
        self.ptr = p

    def upload(self, host: np.ndarray) -> "DeviceBuffer":
        host = np.ascontiguousarray(host)
        if host.nbytes > self.nbytes:
            raise ValueError("host array larger than device buffer")
        self.engine._check(self.engine.lib.gyp_memcpy_h2d(self.engine.ctx, self.ptr, ptr(host), host.nbytes))
        self.engine.sync()   # `host` may be a temporary
        return self

    def download(self, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        self.engine._check(self.engine.lib.gyp_memcpy_d2h(self.engine.ctx, ptr(out), self.ptr, out.nbytes))
        return out

    def free(self) -> None:
        if self.ptr is not None and self.ptr.value:
            self.engine.lib.gyp_free(self.engine.ctx, self.ptr)
            self.ptr = None

    def __del__(self) -> None:
        try:
            self.free()
        except Exception:
            pass


class GypsumEngine:
    def __init__(self, device: int = 0) -> None:
        self.lib = _lib.load()
        h = C.c_void_p()
        rc = self.lib.gyp_create(device, C.byref(h))
        if rc != 0:
            raise GypsumHipError(rc, (self.lib.gyp_last_error(None) or b"").decode())
        self.ctx = h
        self.device = device
        self.fs: Optional[int] = None
        self.n: Optional[int] = None
        self._apply_test_hooks()

    # The library itself reads no GYP_* environment variable.  Test and A/B runs that want to flip a switch of every engine a
    # process creates (tests/, tools/) export GYP_TEST_HOOKS=1 next to the switch; without it the variables below do nothing.
    _ENV_HOOKS = {"GYP_NO_PIPE": "no_pipe", "GYP_NO_SHARED_FWD": "no_shared_fwd", "GYP_NO_GRID_PARTS": "no_grid_parts", "GYP_NO_GRID_FUSED": "no_grid_fused", "GYP_GRID_FUSED_WAVES": "grid_fused_waves", "GYP_NO_ACQ_SPLIT": "no_acq_split",
                  "GYP_NO_SPEC": "no_spec", "GYP_SPEC_DEBUG": "spec_debug", "GYP_ACQ_LANES": "acq_lanes",
                  "GYP_TRACK_CHUNK_MS": "track_chunk_ms", "GYP_WIDEN_WG_PER_CU": "widen_wg_per_cu", "GYP_SYMBOL_TAU": "symbol_tau", "GYP_DLL_PROV_BIAS": "dll_prov_bias",
                  "GYP_SPEC_FAIL_AT": "spec_fail_at", "GYP_SPEC_REDO": "spec_redo", "GYP_SPEC_SUB_MS": "spec_sub_ms", "GYP_NO_EXACT_SHARED": "no_exact_shared", "GYP_PROF_WAVE": "prof_wave",
                  "GYP_TRACK_FINISH_ALL": "track_finish_all"}

    def _apply_test_hooks(self) -> None:
        if os.environ.get("GYP_TEST_HOOKS") != "1":
            return
        for env, name in self._ENV_HOOKS.items():
            v = os.environ.get(env)
            if v is None:
                continue
            self.debug_set(name, float(v) if v.strip() else 1.0)   # a malformed value raises here instead of being read as 0
        if os.environ.get("GYP_SPEC_KAPPA") is not None:
            self.set_params(spec_confidence_kappa=float(os.environ["GYP_SPEC_KAPPA"]))

    def debug_set(self, name: str, value: float) -> None:
        """A/B switches and test hooks of the context (gyp_debug_set; names and ranges in include/gypsum_hip.h)."""
        self._check(self.lib.gyp_debug_set(self.ctx, name.encode(), float(value)))

    def debug_get(self, name: str) -> float:
        v = C.c_double()
        self._check(self.lib.gyp_debug_get(self.ctx, name.encode(), C.byref(v)))
        return float(v.value)

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int) -> None:
        if rc != 0:
            raise GypsumHipError(rc, (self.lib.gyp_last_error(self.ctx) or b"").decode())

    def close(self) -> None:
        if getattr(self, "ctx", None) is not None and self.ctx.value:
            self.lib.gyp_destroy(self.ctx)
            self.ctx = None

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass

    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        self._check(self.lib.gyp_device_name(self.ctx, buf, 256))
        return buf.value.decode()

    def locality(self) -> Dict[str, object]:
        """NUMA node of this engine's GPU and that node's CPUs (gyp_device_locality); node -1 / empty list where the host does not say."""
        node = C.c_int32(-1)
        buf = C.create_string_buffer(8192)
        self._check(self.lib.gyp_device_locality(self.ctx, C.byref(node), buf, 8192))
        text = buf.value.decode()
        cpus = []
        for part in filter(None, text.split(",")):
            a, _, b = part.partition("-")
            cpus.extend(range(int(a), int(b or a) + 1))
        return {"numa_node": int(node.value), "cpulist": text, "cpus": cpus}

    def bind_host_thread_to_gpu_node(self) -> bool:
        """Run the calling thread (and what it allocates from now on) on the CPUs of the GPU's NUMA node; False where unknown."""
        cpus = self.locality()["cpus"]
        if not cpus:
            return False
        try:
            os.sched_setaffinity(0, set(cpus) & os.sched_getaffinity(0) or set(cpus))
            return True
        except OSError:
            return False

    def set_stream(self, hip_stream: Optional[int]) -> None:
        self._check(self.lib.gyp_set_stream(self.ctx, C.c_void_p(hip_stream)))

    def sync(self) -> None:
        self._check(self.lib.gyp_sync(self.ctx))

    def wait_for(self, other: "GypsumEngine") -> None:
        """Work enqueued on this engine from now on waits for everything `other` has enqueued so far (gyp_wait_for)."""
        self._check(self.lib.gyp_wait_for(self.ctx, other.ctx))

    def timer_start(self) -> None:
        self._check(self.lib.gyp_timer_start(self.ctx))

    def timer_stop(self) -> float:
        ms = C.c_float()
        self._check(self.lib.gyp_timer_stop(self.ctx, C.byref(ms)))
        return float(ms.value)

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def host_alloc(self, nbytes: int, dtype=np.uint8) -> np.ndarray:
        """Page-locked host memory as a numpy array (freed with host_free)."""
        p = C.c_void_p()
        self._check(self.lib.gyp_host_alloc(self.ctx, int(nbytes), C.byref(p)))
        buf = (C.c_char * int(nbytes)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.uint8).view(dtype)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr: np.ndarray) -> None:
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is not None:
            self._check(self.lib.gyp_host_free(self.ctx, p))

    def memcpy_h2d_async(self, dst_ptr: int, host: np.ndarray) -> None:
        """Enqueue a host-to-device copy on the engine's stream (asynchronous for page-locked `host`)."""
        self._check(self.lib.gyp_memcpy_h2d(self.ctx, C.c_void_p(dst_ptr), ptr(host), host.nbytes))

    def memcpy_d2h_async(self, host: np.ndarray, src_ptr: int, nbytes: Optional[int] = None) -> None:
        """Enqueue a device-to-host copy on the engine's stream without waiting for it (page-locked `host`; read it after sync())."""
        self._check(self.lib.gyp_memcpy_d2h_async(self.ctx, ptr(host), C.c_void_p(src_ptr), int(host.nbytes if nbytes is None else nbytes)))

    def widen_iq_dev(self, fmt: int, raw_ptr: int, n_words: int, out_ptr: int, scale: float = 1.0) -> None:
        self._check(self.lib.gyp_widen_iq_dev(self.ctx, int(fmt), C.c_void_p(raw_ptr), int(n_words), float(scale), C.c_void_p(out_ptr)))

    # ------------------------------------------------------------------ multi-GPU (gyp_comm_*)
    def resample_iq_dev(self, fmt: int, raw_ptr: int, n_streams: int, in_stride: int, raw_first_sample: int, raw_n_samples: int,
                        scale: float, fs_in: int, taps: int, first_ms: int, n_ms: int, out_stride: int, out_ptr: int) -> None:
        """gyp_resample_iq_dev: output milliseconds first_ms .. first_ms+n_ms-1 at the stream format's rate from file-width words
        at fs_in already in HBM (strides in samples; raw sample 0 is input sample raw_first_sample).  Enqueued, not synchronised."""
        self._check(self.lib.gyp_resample_iq_dev(self.ctx, int(fmt), C.c_void_p(raw_ptr), int(n_streams), int(in_stride),
                                                 int(raw_first_sample), int(raw_n_samples), float(scale), int(fs_in), int(taps),
                                                 int(first_ms), int(n_ms), int(out_stride), C.c_void_p(out_ptr)))

    def resample(self, words: np.ndarray, fmt, fs_in: int, first_ms: int = 0, n_ms: Optional[int] = None, scale: float = 1.0,
                 taps: int = 32) -> np.ndarray:
        """Host convenience: interleaved I,Q `words` of a recording at fs_in (int8 / uint8 / int16 / float32; 2-D = one stream per
        row) -> complex64 output milliseconds first_ms .. first_ms+n_ms-1 at the stream format's rate (default: every output
        millisecond whose first sample lies within the recording).  `fmt` is a GYP_FMT_* code or the words' numpy dtype."""
        from .ingest import _FORMATS
        if self.n is None:
            raise RuntimeError("set_stream_format first")
        w = np.ascontiguousarray(words)
        code = _FORMATS[np.dtype(fmt)] if not isinstance(fmt, (int, np.integer)) else int(fmt)
        if _FORMATS.get(w.dtype) != code:
            raise ValueError(f"words are {w.dtype}, format {code} expects another word type")
        rows = w.reshape(-1, w.shape[-1]) if w.ndim > 1 else w.reshape(1, -1)
        n_streams, n_samples = rows.shape[0], rows.shape[1] // 2
        n_in = int(fs_in) // 1000
        if n_ms is None:
            n_ms = max(0, -(-n_samples // n_in) - int(first_ms))
        out = np.empty((n_streams, n_ms * self.n), dtype=np.complex64)
        if n_ms:
            d_raw = self.alloc(max(1, rows.nbytes)).upload(rows)
            d_out = self.alloc(out.nbytes)
            self.resample_iq_dev(code, d_raw.ptr.value, n_streams, n_samples, 0, n_samples, scale, fs_in, taps, first_ms, n_ms,
                                 n_ms * self.n, d_out.ptr.value)
            self._check(self.lib.gyp_memcpy_d2h(self.ctx, ptr(out), d_out.ptr, out.nbytes))
            d_raw.free()
            d_out.free()
        return out if w.ndim > 1 else out[0]

    def ddc_iq_dev(self, fmt: int, raw_ptr: int, n_streams: int, in_stride: int, raw_first_sample: int, raw_n_samples: int,
                   scale: float, fs_in: int, if_hz: int, taps: int, first_ms: int, n_ms: int, out_stride: int, out_ptr: int) -> None:
        """gyp_ddc_iq_dev: as resample_iq_dev for real words at an IF of if_hz (strides in real samples; raw sample 0 is input
        sample raw_first_sample, which is also the mixer's index).  Enqueued, not synchronised."""
        self._check(self.lib.gyp_ddc_iq_dev(self.ctx, int(fmt), C.c_void_p(raw_ptr), int(n_streams), int(in_stride),
                                            int(raw_first_sample), int(raw_n_samples), float(scale), int(fs_in), int(if_hz), int(taps),
                                            int(first_ms), int(n_ms), int(out_stride), C.c_void_p(out_ptr)))

    def unpack_iq_dev(self, packing, raw_ptr: int, n_streams: int, in_stride_bytes: int, bit0: int, n_samples: int, scale: float,
                      out_stride: int, out_ptr: int) -> None:
        """gyp_unpack_iq_dev: packed I,Q words (gypsum_amd.packing.Packing) in HBM -> complex64 at their own rate; stream s starts
        at byte raw_ptr + s * in_stride_bytes, its sample 0 bit0 bits into that byte.  Enqueued, not synchronised."""
        rec = packing.record()
        self._check(self.lib.gyp_unpack_iq_dev(self.ctx, ptr(rec), C.c_void_p(raw_ptr), int(n_streams), int(in_stride_bytes), int(bit0),
                                               int(n_samples), float(scale), int(out_stride), C.c_void_p(out_ptr)))

    def resample_packed_dev(self, packing, raw_ptr: int, n_streams: int, in_stride_bytes: int, bit0: int, raw_first_sample: int,
                            raw_n_samples: int, scale: float, fs_in: int, if_hz: int, taps: int, first_ms: int, n_ms: int,
                            out_stride: int, out_ptr: int) -> None:
        """gyp_resample_packed_dev: resample_iq_dev (an I,Q packing, if_hz 0) or ddc_iq_dev (a real packing) on packed words; strides
        in bytes, the buffer's sample 0 (input sample raw_first_sample) bit0 bits into its first byte.  Enqueued, not synchronised."""
        rec = packing.record()
        self._check(self.lib.gyp_resample_packed_dev(self.ctx, ptr(rec), C.c_void_p(raw_ptr), int(n_streams), int(in_stride_bytes),
                                                     int(bit0), int(raw_first_sample), int(raw_n_samples), float(scale), int(fs_in),
                                                     int(if_hz), int(taps), int(first_ms), int(n_ms), int(out_stride), C.c_void_p(out_ptr)))

    def ddc(self, words: np.ndarray, fmt, fs_in: int, if_hz: int, first_ms: int = 0, n_ms: Optional[int] = None, scale: float = 1.0,
            taps: int = 0) -> np.ndarray:
        """Host convenience: real `words` of a recording at fs_in with its band at if_hz (int8 / uint8 / int16 / float32; 2-D = one
        stream per row) -> complex64 baseband output milliseconds first_ms .. first_ms+n_ms-1 at the stream format's rate (default:
        every output millisecond whose first sample lies within the recording).  `fmt` is a GYP_FMT_* code or the words' dtype."""
        from .ingest import _FORMATS
        if self.n is None:
            raise RuntimeError("set_stream_format first")
        w = np.ascontiguousarray(words)
        code = _FORMATS[np.dtype(fmt)] if not isinstance(fmt, (int, np.integer)) else int(fmt)
        if _FORMATS.get(w.dtype) != code:
            raise ValueError(f"words are {w.dtype}, format {code} expects another word type")
        rows = w.reshape(-1, w.shape[-1]) if w.ndim > 1 else w.reshape(1, -1)
        n_streams, n_samples = rows.shape
        n_in = int(fs_in) // 1000
        if n_ms is None:
            n_ms = max(0, -(-n_samples // n_in) - int(first_ms))
        out = np.empty((n_streams, n_ms * self.n), dtype=np.complex64)
        if n_ms:
            d_raw = self.alloc(max(1, rows.nbytes)).upload(rows)
            d_out = self.alloc(out.nbytes)
            self.ddc_iq_dev(code, d_raw.ptr.value, n_streams, n_samples, 0, n_samples, scale, fs_in, if_hz, taps, first_ms, n_ms,
                            n_ms * self.n, d_out.ptr.value)
            self._check(self.lib.gyp_memcpy_d2h(self.ctx, ptr(out), d_out.ptr, out.nbytes))
            d_raw.free()
            d_out.free()
        return out if w.ndim > 1 else out[0]

    def iq_stats_dev(self, iq_ptr: int, n_streams: int, stream_stride: int, n_ms: int, samples_per_ms: int, clip_level: float,
                     out_ptr: int) -> None:
        """gyp_iq_stats_dev: one gyp_iq_stats record per (stream, millisecond) of complex64 samples in HBM (any samples_per_ms, no
        stream format needed), stream-major into out_ptr.  Enqueued, not synchronised."""
        self._check(self.lib.gyp_iq_stats_dev(self.ctx, C.c_void_p(iq_ptr), int(n_streams), int(stream_stride), int(n_ms),
                                              int(samples_per_ms), float(clip_level), C.c_void_p(out_ptr)))

    def condition_iq_dev(self, in_ptr: int, out_ptr: int, n_streams: int, stream_stride: int, n_samples: int, levels) -> None:
        """gyp_condition_iq_dev: out = (in - dc) * gain in float32, stream s with levels[s] (gypsum_amd.level.IqLevel); out_ptr may
        equal in_ptr.  Enqueued, not synchronised."""
        from .level import level_records
        recs = level_records(levels)
        if len(recs) != int(n_streams):
            raise ValueError(f"{len(recs)} levels for {n_streams} streams")
        self._check(self.lib.gyp_condition_iq_dev(self.ctx, C.c_void_p(in_ptr), C.c_void_p(out_ptr), int(n_streams), int(stream_stride),
                                                  int(n_samples), ptr(recs)))

    def iq_stats(self, iq: np.ndarray, samples_per_ms: int, clip_level: float = 0.0) -> np.ndarray:
        """Host convenience: the per-millisecond records (gypsum_amd.level.STATS_DTYPE) of complex64 `iq` (2-D = one stream per
        row), shape ([n_streams,] n_ms) over the whole milliseconds of samples_per_ms samples it holds."""
        x = _as_iq(iq)
        rows = x.reshape(-1, x.shape[-1]) if x.ndim > 1 else x.reshape(1, -1)
        n_streams, n_ms = rows.shape[0], rows.shape[1] // int(samples_per_ms)
        out = np.zeros((n_streams, n_ms), dtype=_lib.IQ_STATS)
        if n_ms:
            d_iq = self.alloc(rows.nbytes).upload(rows)
            d_out = self.alloc(out.nbytes)
            self.iq_stats_dev(d_iq.ptr.value, n_streams, rows.shape[1], n_ms, samples_per_ms, clip_level, d_out.ptr.value)
            self._check(self.lib.gyp_memcpy_d2h(self.ctx, ptr(out), d_out.ptr, out.nbytes))
            d_iq.free()
            d_out.free()
        return out if x.ndim > 1 else out[0]

    def condition_iq(self, iq: np.ndarray, levels) -> np.ndarray:
        """Host convenience: (iq - dc) * gain in float32 on the device, complex64 `iq` (2-D = one stream per row, one level each)."""
        x = _as_iq(iq)
        rows = x.reshape(-1, x.shape[-1]) if x.ndim > 1 else x.reshape(1, -1)
        out = np.empty_like(rows)
        if rows.size:
            d = self.alloc(rows.nbytes).upload(rows)
            self.condition_iq_dev(d.ptr.value, d.ptr.value, rows.shape[0], rows.shape[1], rows.shape[1], levels)
            self._check(self.lib.gyp_memcpy_d2h(self.ctx, ptr(out), d.ptr, out.nbytes))
            d.free()
        return out if x.ndim > 1 else out[0]

    def iq_tones_dev(self, iq_ptr: int, n_streams: int, stream_stride: int, first_sample_index: int, n_blocks: int, block_samples: int,
                     fs_hz: int, freqs_hz, window: int, out_ptr: int) -> None:
        """gyp_iq_tones_dev: one gyp_tone_rec per (stream, block, frequency) of complex64 samples in HBM, stream-major, then block, then
        frequency, into out_ptr.  Enqueued, not synchronised."""
        f = np.ascontiguousarray(freqs_hz, dtype=np.int64).reshape(-1)
        self._check(self.lib.gyp_iq_tones_dev(self.ctx, C.c_void_p(iq_ptr), int(n_streams), int(stream_stride), int(first_sample_index),
                                              int(n_blocks), int(block_samples), int(fs_hz), ptr(f), len(f), int(window), C.c_void_p(out_ptr)))

    def notch_iq_dev(self, in_ptr: int, out_ptr: int, n_streams: int, stream_stride: int, first_sample_index: int, n_ms: int,
                     samples_per_ms: int, fs_hz: int, tones) -> None:
        """gyp_notch_iq_dev: the tones of stream s (gypsum_amd.notch.notch_records) projected out of every millisecond, in list order;
        out_ptr may equal in_ptr.  Enqueued, not synchronised."""
        from .notch import notch_records
        recs = notch_records(tones, n_streams)
        if len(recs) != int(n_streams):
            raise ValueError(f"{len(recs)} tone lists for {n_streams} streams")
        self._check(self.lib.gyp_notch_iq_dev(self.ctx, C.c_void_p(in_ptr), C.c_void_p(out_ptr), int(n_streams), int(stream_stride),
                                              int(first_sample_index), int(n_ms), int(samples_per_ms), int(fs_hz), ptr(recs)))

    def iq_tones(self, iq: np.ndarray, fs_hz: int, freqs_hz, block_samples: int, window: int = 0, first_sample_index: int = 0) -> np.ndarray:
        """Host convenience: the records (gypsum_amd.notch.TONE_DTYPE) of complex64 `iq` (2-D = one stream per row), shape
        ([n_streams,] n_blocks, n_freq) over the whole blocks of block_samples samples it holds."""
        x = _as_iq(iq)
        rows = x.reshape(-1, x.shape[-1]) if x.ndim > 1 else x.reshape(1, -1)
        f = np.ascontiguousarray(freqs_hz, dtype=np.int64).reshape(-1)
        n_streams, n_blocks = rows.shape[0], rows.shape[1] // int(block_samples)
        out = np.zeros((n_streams, n_blocks, len(f)), dtype=_lib.TONE_REC)
        if out.size:
            d_iq = self.alloc(rows.nbytes).upload(rows)
            d_out = self.alloc(out.nbytes)
            self.iq_tones_dev(d_iq.ptr.value, n_streams, rows.shape[1], first_sample_index, n_blocks, block_samples, fs_hz, f, window,
                              d_out.ptr.value)
            self._check(self.lib.gyp_memcpy_d2h(self.ctx, ptr(out), d_out.ptr, out.nbytes))
            d_iq.free()
            d_out.free()
        return out if x.ndim > 1 else out[0]

    def notch_iq(self, iq: np.ndarray, fs_hz: int, samples_per_ms: int, tones, first_sample_index: int = 0) -> np.ndarray:
        """Host convenience: complex64 `iq` (2-D = one stream per row, one tone list each or one for all) with the tones projected out
        of every whole millisecond on the device; a trailing part of a millisecond is returned as it is."""
        x = _as_iq(iq)
        rows = x.reshape(-1, x.shape[-1]) if x.ndim > 1 else x.reshape(1, -1)
        out = rows.copy()
        n_ms = rows.shape[1] // int(samples_per_ms)
        if n_ms:
            d = self.alloc(rows.nbytes).upload(rows)
            self.notch_iq_dev(d.ptr.value, d.ptr.value, rows.shape[0], rows.shape[1], first_sample_index, n_ms, samples_per_ms, fs_hz, tones)
            self._check(self.lib.gyp_memcpy_d2h(self.ctx, ptr(out), d.ptr, out.nbytes))
            d.free()
        return out if x.ndim > 1 else out[0]

    def blank_iq_dev(self, in_ptr: int, out_ptr: int, n_streams: int, stream_stride: int, n_ms: int, samples_per_ms: int, blankers,
                     counts_ptr: int = 0) -> None:
        """gyp_blank_iq_dev: per millisecond, every sample whose power about the centre reaches the threshold and `guard` samples on
        either side become the centre, stream s with blankers[s] (gypsum_amd.blanker.Blanker); out_ptr may equal in_ptr; counts_ptr
        (0: none) receives n_streams x n_ms int32 counts of blanked samples.  Enqueued, not synchronised."""
        from .blanker import blanker_records
        recs = blanker_records(blankers, n_streams)
        if len(recs) != max(1, int(n_streams)):   # (a count below 1 is the library's to refuse)
            raise ValueError(f"{len(recs)} blankers for {n_streams} streams")
        self._check(self.lib.gyp_blank_iq_dev(self.ctx, C.c_void_p(in_ptr), C.c_void_p(out_ptr), int(n_streams), int(stream_stride),
                                              int(n_ms), int(samples_per_ms), ptr(recs), C.c_void_p(counts_ptr or None)))

    def power_hist_dev(self, iq_ptr: int, n_streams: int, stream_stride: int, n_samples: int, centers, hist_ptr: int) -> None:
        """gyp_iq_power_hist_dev: n_streams x 2048 uint32 counts of the samples' power about centers[s] (pairs of floats; None: 0) in
        eighth-octave bins into hist_ptr, which is zeroed first.  Enqueued, not synchronised."""
        c = None if centers is None else np.ascontiguousarray(centers, dtype=np.float32).reshape(-1)
        if c is not None and len(c) != 2 * int(n_streams):
            raise ValueError(f"{len(c)} centre components for {n_streams} streams")
        self._check(self.lib.gyp_iq_power_hist_dev(self.ctx, C.c_void_p(iq_ptr), int(n_streams), int(stream_stride), int(n_samples),
                                                   ptr(c), C.c_void_p(hist_ptr)))

    def blank_iq(self, iq: np.ndarray, samples_per_ms: int, blankers):
        """Host convenience: (complex64 `iq` blanked over its whole milliseconds on the device, int32 counts [[n_streams,] n_ms]);
        2-D = one stream per row, one blanker each or one for all; a trailing part of a millisecond is returned as it is."""
        x = _as_iq(iq)
        rows = x.reshape(-1, x.shape[-1]) if x.ndim > 1 else x.reshape(1, -1)
        out = rows.copy()
        n_ms = rows.shape[1] // int(samples_per_ms)
        counts = np.zeros((rows.shape[0], n_ms), dtype=np.int32)
        if n_ms:
            d = self.alloc(rows.nbytes).upload(rows)
            d_counts = self.alloc(counts.nbytes)
            self.blank_iq_dev(d.ptr.value, d.ptr.value, rows.shape[0], rows.shape[1], n_ms, samples_per_ms, blankers, d_counts.ptr.value)
            self._check(self.lib.gyp_memcpy_d2h(self.ctx, ptr(out), d.ptr, out.nbytes))
            self._check(self.lib.gyp_memcpy_d2h(self.ctx, ptr(counts), d_counts.ptr, counts.nbytes))
            d.free()
            d_counts.free()
        return (out, counts) if x.ndim > 1 else (out[0], counts[0])

    def power_hist(self, iq: np.ndarray, centers=None) -> np.ndarray:
        """Host convenience: the uint32 histogram(s) [[n_streams,] 2048] of complex64 `iq` (2-D = one stream per row) about `centers`
        (one complex number or (re, im) pair per stream; None: 0)."""
        x = _as_iq(iq)
        rows = x.reshape(-1, x.shape[-1]) if x.ndim > 1 else x.reshape(1, -1)
        if centers is not None:
            c = np.asarray(centers)
            centers = np.stack([c.real, c.imag], axis=-1) if np.iscomplexobj(c) else c
        out = np.zeros((rows.shape[0], _lib.GYP_POWER_HIST_BINS), dtype=np.uint32)
        if rows.shape[1]:
            d_iq = self.alloc(rows.nbytes).upload(rows)
            d_out = self.alloc(out.nbytes)
            self.power_hist_dev(d_iq.ptr.value, rows.shape[0], rows.shape[1], rows.shape[1], centers, d_out.ptr.value)
            self._check(self.lib.gyp_memcpy_d2h(self.ctx, ptr(out), d_out.ptr, out.nbytes))
            d_iq.free()
            d_out.free()
        return out if x.ndim > 1 else out[0]

    def excise_iq_dev(self, in_ptr: int, out_ptr: int, n_streams: int, stream_stride: int, n_ms: int, samples_per_ms: int, excisors,
                      counts_ptr: int = 0, masks_ptr: int = 0) -> None:
        """gyp_excise_iq_dev: per millisecond, half-overlapped 256-point transforms; what the bins that reach the threshold and `guard`
        bins on either side held is subtracted, stream s with excisors[s] (gypsum_amd.excisor.Excisor); out_ptr may equal in_ptr;
        counts_ptr (0: none) receives n_streams x n_ms int32 counts of excised (frame, bin) cells, masks_ptr (0: none) four uint64
        words per (stream, millisecond, frame).  Enqueued, not synchronised."""
        from .excisor import excisor_records
        recs = excisor_records(excisors, n_streams)
        if len(recs) != max(1, int(n_streams)):   # (a count below 1 is the library's to refuse)
            raise ValueError(f"{len(recs)} excisors for {n_streams} streams")
        self._check(self.lib.gyp_excise_iq_dev(self.ctx, C.c_void_p(in_ptr), C.c_void_p(out_ptr), int(n_streams), int(stream_stride),
                                               int(n_ms), int(samples_per_ms), ptr(recs), C.c_void_p(counts_ptr or None),
                                               C.c_void_p(masks_ptr or None)))

    def spectrum_hist_dev(self, iq_ptr: int, n_streams: int, stream_stride: int, n_ms: int, samples_per_ms: int, hist_ptr: int) -> None:
        """gyp_iq_spectrum_hist_dev: n_streams x 2048 uint32 counts of the bin powers of the frames that lie inside their millisecond,
        in eighth-octave bins, into hist_ptr, which is zeroed first.  Enqueued, not synchronised."""
        self._check(self.lib.gyp_iq_spectrum_hist_dev(self.ctx, C.c_void_p(iq_ptr), int(n_streams), int(stream_stride), int(n_ms),
                                                      int(samples_per_ms), C.c_void_p(hist_ptr)))

    def excise_iq(self, iq: np.ndarray, samples_per_ms: int, excisors):
        """Host convenience: (complex64 `iq` excised over its whole milliseconds on the device, int32 counts [[n_streams,] n_ms],
        uint64 masks [[n_streams,] n_ms, frames, 4]); 2-D = one stream per row, one excisor each or one for all; a trailing part of
        a millisecond is returned as it is."""
        from .excisor import n_frames
        x = _as_iq(iq)
        rows = x.reshape(-1, x.shape[-1]) if x.ndim > 1 else x.reshape(1, -1)
        out = rows.copy()
        n_ms = rows.shape[1] // int(samples_per_ms)
        counts = np.zeros((rows.shape[0], n_ms), dtype=np.int32)
        masks = np.zeros((rows.shape[0], n_ms, n_frames(samples_per_ms), 4), dtype=np.uint64)
        if n_ms:
            d = self.alloc(rows.nbytes).upload(rows)
            d_counts, d_masks = self.alloc(counts.nbytes), self.alloc(masks.nbytes)
            self.excise_iq_dev(d.ptr.value, d.ptr.value, rows.shape[0], rows.shape[1], n_ms, samples_per_ms, excisors, d_counts.ptr.value,
                               d_masks.ptr.value)
            self._check(self.lib.gyp_memcpy_d2h(self.ctx, ptr(out), d.ptr, out.nbytes))
            self._check(self.lib.gyp_memcpy_d2h(self.ctx, ptr(counts), d_counts.ptr, counts.nbytes))
            self._check(self.lib.gyp_memcpy_d2h(self.ctx, ptr(masks), d_masks.ptr, masks.nbytes))
            for b in (d, d_counts, d_masks):
                b.free()
        return (out, counts, masks) if x.ndim > 1 else (out[0], counts[0], masks[0])

    def spectrum_hist(self, iq: np.ndarray, samples_per_ms: int) -> np.ndarray:
        """Host convenience: the uint32 histogram(s) [[n_streams,] 2048] of the bin powers of complex64 `iq` (2-D = one stream per
        row) over its whole milliseconds of samples_per_ms >= 256 samples."""
        x = _as_iq(iq)
        rows = x.reshape(-1, x.shape[-1]) if x.ndim > 1 else x.reshape(1, -1)
        out = np.zeros((rows.shape[0], _lib.GYP_POWER_HIST_BINS), dtype=np.uint32)
        d_iq = self.alloc(max(rows.nbytes, 8)).upload(rows)
        d_out = self.alloc(out.nbytes)
        try:
            self.spectrum_hist_dev(d_iq.ptr.value, rows.shape[0], rows.shape[1], rows.shape[1] // int(samples_per_ms), samples_per_ms, d_out.ptr.value)
            self._check(self.lib.gyp_memcpy_d2h(self.ctx, ptr(out), d_out.ptr, out.nbytes))
        finally:
            d_iq.free()
            d_out.free()
        return out if x.ndim > 1 else out[0]

    def track_quality_dev(self, rec_ptr: int, n_chan: int, chan_stride: int, n_ms: int, window_ms: int, out_ptr: int,
                          bit_offsets=None) -> None:
        """gyp_track_quality_dev: one gyp_quality_sums record per (channel, window of window_ms records) of tracking records in HBM,
        channel-major into out_ptr; bit_offsets: per channel -1..19, None = no groups.  Enqueued, not synchronised."""
        from .quality import bit_offset_records
        b = bit_offset_records(bit_offsets, n_chan)
        self._check(self.lib.gyp_track_quality_dev(self.ctx, C.c_void_p(rec_ptr), int(n_chan), int(chan_stride), int(n_ms),
                                                   int(window_ms), ptr(b), C.c_void_p(out_ptr)))

    def track_quality(self, records: np.ndarray, window_ms: int, bit_offsets=None) -> np.ndarray:
        """Host convenience (gyp_track_quality): the sums (gypsum_amd.quality.SUMS_DTYPE) of `records` (TRACK_REC, 2-D = one channel
        per row), shape ([n_chan,] ceil(n_ms / window_ms))."""
        from .quality import bit_offset_records
        r = np.ascontiguousarray(records, dtype=TRACK_REC)
        rows = r if r.ndim > 1 else r.reshape(1, -1)
        n_chan, n_ms = rows.shape
        b = bit_offset_records(bit_offsets, n_chan)
        out = np.zeros((n_chan, -(-n_ms // int(window_ms)) if int(window_ms) > 0 else 0), dtype=_lib.QUALITY_SUMS)
        self._check(self.lib.gyp_track_quality(self.ctx, ptr(rows), n_chan, n_ms, n_ms, int(window_ms), ptr(b), ptr(out)))
        return out if r.ndim > 1 else out[0]

    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(_lib.GYP_COMM_ID_BYTES)
        rc = self.lib.gyp_comm_unique_id(buf)
        if rc != 0:
            raise GypsumHipError(rc, (self.lib.gyp_last_error(None) or b"").decode())
        return buf.raw

    def comm_init(self, rank: int, world: int, unique_id: Optional[bytes]) -> None:
        """One RCCL communicator per context (`unique_id` from rank 0's comm_unique_id(), 128 bytes); None with
        world == 1 declares a single-process world without RCCL."""
        uid = C.create_string_buffer(unique_id, _lib.GYP_COMM_ID_BYTES) if unique_id is not None else None
        self._check(self.lib.gyp_comm_init(self.ctx, int(rank), int(world), uid))

    def comm_destroy(self) -> None:
        self._check(self.lib.gyp_comm_destroy(self.ctx))

    def comm_info(self) -> Dict[str, int]:
        r, w, u = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.gyp_comm_info(self.ctx, C.byref(r), C.byref(w), C.byref(u)))
        return {"rank": r.value, "world": w.value, "uses_rccl": u.value}

    def allgather_dev(self, send_ptr: int, recv_ptr: int, bytes_per_rank: int) -> None:
        """ncclAllGather of opaque record bytes on the engine's stream (device copy in a single-process world)."""
        self._check(self.lib.gyp_allgather_dev(self.ctx, C.c_void_p(send_ptr), C.c_void_p(recv_ptr), int(bytes_per_rank)))

    def set_stream_format(self, samples_per_second: int, samples_per_prn_transmission: int) -> None:
        self._check(self.lib.gyp_set_stream_format(self.ctx, int(samples_per_second), int(samples_per_prn_transmission)))
        self.fs, self.n = int(samples_per_second), int(samples_per_prn_transmission)

    # ------------------------------------------------------------------ correlation cells
    def correlate_cells(self, iq: np.ndarray, n_streams: int, n_ms: int, cells: np.ndarray, integration: int,
                        want_profiles: bool = False) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """iq: complex64[n_streams * n_ms * N] stream-major.  cells: CELL_DESC records."""
        iq = _iq_arg(iq, (n_streams, n_ms, self.n))
        cells = np.ascontiguousarray(cells, dtype=CELL_DESC)
        out = np.zeros(len(cells), dtype=CELL)
        prof = None
        if want_profiles:
            prof = np.zeros((len(cells), self.n), dtype=np.complex64 if integration == GYP_COHERENT else np.float32)
        self._check(self.lib.gyp_correlate_cells(self.ctx, ptr(iq), n_streams, n_ms, ptr(cells), len(cells),
                                                  integration, ptr(out), ptr(prof)))
        return out, prof

    def correlate_grid(self, iq: np.ndarray, n_streams: int, n_ms: int, sat_ids: Sequence[int], doppler_hz: Sequence[float],
                       integration: int) -> np.ndarray:
        """Flat grid with shared Doppler bins: CELL records [n_streams, n_sats, n_bins]."""
        iq = _iq_arg(iq, (n_streams, n_ms, self.n))
        ids, bins = _ids(sat_ids), _bins(doppler_hz)
        out = np.zeros((n_streams, len(ids), len(bins)), dtype=CELL)
        self._check(self.lib.gyp_correlate_grid(self.ctx, ptr(iq), n_streams, n_ms, ptr(ids), len(ids), ptr(bins), len(bins),
                                                 integration, ptr(out)))
        return out

    def correlate_grid_dev(self, iq_ptr: int, n_streams: int, stream_stride: int, n_ms: int, sat_ids: Sequence[int],
                           doppler_hz: Sequence[float], integration: int, out_ptr: int) -> None:
        ids, bins = _ids(sat_ids), _bins(doppler_hz)
        self._check(self.lib.gyp_correlate_grid_dev(self.ctx, C.c_void_p(iq_ptr), n_streams, stream_stride, n_ms, ptr(ids),
                                                     len(ids), ptr(bins), len(bins), integration, C.c_void_p(out_ptr)))

    def grid_best_bins_dev(self, cells_ptr: int, n_rows: int, n_bins: int, out_ptr: int) -> None:
        """acquisition.py:180-189 per (stream, satellite) row of a flat grid's records, on the device (BEST_BIN records)."""
        self._check(self.lib.gyp_grid_best_bins_dev(self.ctx, C.c_void_p(cells_ptr), int(n_rows), int(n_bins), C.c_void_p(out_ptr)))

    def grid_best_bins_refined_dev(self, iq_ptr: int, n_streams: int, stream_stride: int, n_ms: int, sat_ids: Sequence[int],
                                   doppler_hz: Sequence[float], integration: int, cells_ptr: int, out_ptr: int) -> int:
        """The same selection with the float64 tie-break between near-equal bins (gyp_grid_best_bins_refined_dev): the grid as
        correlate_grid_dev took it + the records it wrote.  Returns the number of rows decided in float64."""
        ids, bins = _ids(sat_ids), _bins(doppler_hz)
        self._check(self.lib.gyp_grid_best_bins_refined_dev(self.ctx, C.c_void_p(iq_ptr), n_streams, stream_stride, n_ms, ptr(ids), len(ids),
                                                             ptr(bins), len(bins), integration, C.c_void_p(cells_ptr), C.c_void_p(out_ptr)))
        return int(self.debug_get("last_grid_refined_rows"))

    def cell_strength(self, cells: np.ndarray) -> np.ndarray:
        """utils.py:111-116 on the reduced record, float64."""
        pk = cells["peak"].astype(np.float64)
        return pk / ((cells["sum"] - cells["n_max"] * pk) / (self.n - cells["n_max"]))

    # ------------------------------------------------------------------ acquisition
    def acquire(self, iq: np.ndarray, n_streams: int, n_ms: int, sat_ids: Sequence[int]) -> np.ndarray:
        iq = _iq_arg(iq, (n_streams, n_ms, self.n))
        ids = _ids(sat_ids)
        out = np.zeros(n_streams * len(ids), dtype=ACQ_RESULT)
        self._check(self.lib.gyp_acquire(self.ctx, ptr(iq), n_streams, n_ms, ptr(ids), len(ids), ptr(out)))
        return out

    def search_level(self, iq: np.ndarray, n_streams: int, n_ms: int, sat_ids: Sequence[int], center_hz: float,
                     spread_hz: float) -> np.ndarray:
        """One level of the search (acquisition.py:154-190): best bin, its arg-max and strength per (stream, satellite)."""
        iq = _iq_arg(iq, (n_streams, n_ms, self.n))
        ids = _ids(sat_ids)
        out = np.zeros(n_streams * len(ids), dtype=ACQ_RESULT)
        self._check(self.lib.gyp_search_level(self.ctx, ptr(iq), n_streams, n_ms, ptr(ids), len(ids), float(center_hz),
                                               float(spread_hz), ptr(out)))
        return out

    # ------------------------------------------------------------------ tunables (gyp_params)
    def get_params(self) -> dict:
        rec = np.zeros(1, dtype=PARAMS)
        self._check(self.lib.gyp_get_params(self.ctx, ptr(rec)))
        return {k: float(rec[0][k]) for k in PARAMS.names}

    def set_params(self, **changes: float) -> dict:
        """Change some of the reference's tunables (names as in gyp_params); returns the full set now in force."""
        rec = np.zeros(1, dtype=PARAMS)
        self._check(self.lib.gyp_get_params(self.ctx, ptr(rec)))
        for k, v in changes.items():
            if k not in PARAMS.names:
                raise KeyError(k)
            rec[0][k] = float(v)
        self._check(self.lib.gyp_set_params(self.ctx, ptr(rec)))
        return {k: float(rec[0][k]) for k in PARAMS.names}

    def acquire_dev(self, iq_ptr: int, n_streams: int, stream_stride: int, n_ms: int, sat_ids: Sequence[int],
                    out_ptr: int) -> None:
        """Device-pointer form (asynchronous on the engine's stream): out_ptr receives n_streams*len(sat_ids) records."""
        ids = _ids(sat_ids)
        self._check(self.lib.gyp_acquire_dev(self.ctx, C.c_void_p(iq_ptr), n_streams, stream_stride, n_ms, ptr(ids),
                                              len(ids), C.c_void_p(out_ptr)))

    # ------------------------------------------------------------------ weak-signal acquisition (hybrid search)
    def correlate_grid_hybrid(self, iq: np.ndarray, n_streams: int, coherent_ms: int, n_blocks: int, flags: int, sat_ids: Sequence[int],
                              doppler_hz: Sequence[float]) -> np.ndarray:
        """Flat grid of the hybrid coherent/non-coherent search: HYBRID_CELL records [n_streams, n_sats, n_bins] from
        n_blocks blocks of coherent_ms milliseconds (iq: complex64[n_streams * n_blocks * coherent_ms * N], stream-major)."""
        iq = _iq_arg(iq, (n_streams, n_blocks, coherent_ms, self.n), check=coherent_ms >= 1 and n_blocks >= 1)
        ids, bins = _ids(sat_ids), _bins(doppler_hz)
        out = np.zeros((n_streams, len(ids), len(bins)), dtype=_lib.HYBRID_CELL)
        self._check(self.lib.gyp_correlate_grid_hybrid(self.ctx, ptr(iq), n_streams, int(coherent_ms), int(n_blocks), int(flags), ptr(ids), len(ids),
                                                        ptr(bins), len(bins), ptr(out)))
        return out

    def correlate_grid_hybrid_dev(self, iq_ptr: int, n_streams: int, stream_stride: int, coherent_ms: int, n_blocks: int, flags: int,
                                  sat_ids: Sequence[int], doppler_hz: Sequence[float], out_ptr: int) -> None:
        ids, bins = _ids(sat_ids), _bins(doppler_hz)
        self._check(self.lib.gyp_correlate_grid_hybrid_dev(self.ctx, C.c_void_p(iq_ptr), n_streams, stream_stride, int(coherent_ms), int(n_blocks),
                                                            int(flags), ptr(ids), len(ids), ptr(bins), len(bins), C.c_void_p(out_ptr)))

    def acquire_weak(self, iq: np.ndarray, n_streams: int, coherent_ms: int, n_blocks: int, flags: int, sat_ids: Sequence[int],
                     center_hz: float = 0.0, spread_hz: float = 7000.0, fine_step_hz: float = 10.0) -> np.ndarray:
        """The two-level hybrid search per (stream, satellite): WEAK_RESULT records, stream-major, satellites in the order given.
        The threshold on `z` is the caller's."""
        iq = _iq_arg(iq, (n_streams, n_blocks, coherent_ms, self.n), check=coherent_ms >= 1 and n_blocks >= 1)
        ids = _ids(sat_ids)
        out = np.zeros(n_streams * len(ids), dtype=_lib.WEAK_RESULT)
        self._check(self.lib.gyp_acquire_weak(self.ctx, ptr(iq), n_streams, int(coherent_ms), int(n_blocks), int(flags), float(center_hz),
                                               float(spread_hz), float(fine_step_hz), ptr(ids), len(ids), ptr(out)))
        return out

    def acquire_weak_dev(self, iq_ptr: int, n_streams: int, stream_stride: int, coherent_ms: int, n_blocks: int, flags: int,
                         sat_ids: Sequence[int], center_hz: float, spread_hz: float, fine_step_hz: float, out_ptr: int) -> None:
        """Device-pointer form: only enqueues on the engine's stream."""
        ids = _ids(sat_ids)
        self._check(self.lib.gyp_acquire_weak_dev(self.ctx, C.c_void_p(iq_ptr), n_streams, stream_stride, int(coherent_ms), int(n_blocks), int(flags),
                                                   float(center_hz), float(spread_hz), float(fine_step_hz), ptr(ids), len(ids), C.c_void_p(out_ptr)))

    def hybrid_stats(self, cells: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """(z, peak_ratio) of HYBRID_CELL records, float64 (gyp_hybrid_stats; see hybrid_stats below)."""
        return hybrid_stats(cells)

    # ------------------------------------------------------------------ weak-signal hand-over (search -> refine -> weak bank)
    def refine_weak(self, iq: np.ndarray, n_streams: int, first_ms: int, results: np.ndarray, params=None,
                    want_prompts: bool = False) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """gyp_weak_refine: the sub-Hz Doppler, the bit edge and the carrier phase of each WEAK_RESULT record from the open-loop prompts
        of iq (complex64[n_streams * n_ms * N], stream-major, 40..2000 whole milliseconds from the absolute millisecond first_ms).
        (WEAK_REFINED[len(results)], the complex64 prompts [len(results), n_ms] or None).  params: a _records.WeakRefineParams or a
        WEAK_REFINE_PARAMS record (None: the defaults)."""
        iq = _as_iq(iq).reshape(-1)
        n_ms = iq.size // (max(int(n_streams), 1) * self.n)
        if iq.size != max(int(n_streams), 1) * n_ms * self.n:
            raise ValueError("a whole number of milliseconds per stream expected")
        res = np.ascontiguousarray(results, dtype=_lib.WEAK_RESULT).reshape(-1)
        prm = _refine_params(params)
        out = np.zeros(len(res), dtype=_lib.WEAK_REFINED)
        prompts = np.zeros((len(res), n_ms), dtype=np.complex64) if want_prompts else None
        self._check(self.lib.gyp_weak_refine(self.ctx, ptr(iq) if iq.size else None, int(n_streams), int(first_ms), n_ms, ptr(res) if res.size else None,
                                              len(res), ptr(prm), ptr(out), ptr(prompts)))
        return out, prompts

    def refine_weak_dev(self, iq_ptr: int, n_streams: int, stream_stride: int, first_ms: int, n_ms: int, results: np.ndarray, out_ptr: int,
                        params=None, prompts_ptr: int = 0) -> None:
        """Device-pointer form: waits for the stream once, after uploading the candidates, then only enqueues."""
        res = np.ascontiguousarray(results, dtype=_lib.WEAK_RESULT).reshape(-1)
        self._check(self.lib.gyp_weak_refine_dev(self.ctx, C.c_void_p(iq_ptr or None), int(n_streams), int(stream_stride), int(first_ms), int(n_ms),
                                                  ptr(res) if res.size else None, len(res), ptr(_refine_params(params)), C.c_void_p(out_ptr or None),
                                                  C.c_void_p(prompts_ptr or None)))

    # ------------------------------------------------------------------ weak-signal measurement (refine -> measure -> weak bank)
    def measure_weak(self, iq: np.ndarray, n_streams: int, first_ms: int, refined: np.ndarray, params=None,
                     want_sums: bool = False) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[np.ndarray], Optional[np.ndarray]]:
        """gyp_weak_measure: the fractional code phase and the C/N0 of each WEAK_REFINED record from the early / prompt / late sums of
        iq (complex64[n_streams * n_ms * N], stream-major, 40..2000 whole milliseconds from the absolute millisecond first_ms).
        (WEAK_MEASURED[len(refined)], and with want_sums the WEAK_MS_REC sums [len(refined), passes, n_ms], the float64 W_m of the same
        shape and the WEAK_MEASURE_FOLD records [len(refined), passes]; None each otherwise).  params: a _records.WeakMeasureParams or a
        WEAK_MEASURE_PARAMS record (None: the defaults)."""
        iq = _as_iq(iq).reshape(-1)
        n_ms = iq.size // (max(int(n_streams), 1) * self.n)
        if iq.size != max(int(n_streams), 1) * n_ms * self.n:
            raise ValueError("a whole number of milliseconds per stream expected")
        ref = np.ascontiguousarray(refined, dtype=_lib.WEAK_REFINED).reshape(-1)
        prm = _measure_params(params)
        passes = max(1, min(4, int(prm[0]["passes"]))) if prm is not None else 2
        out = np.zeros(len(ref), dtype=_lib.WEAK_MEASURED)
        sums = np.zeros((len(ref), passes, n_ms), dtype=_lib.WEAK_MS_REC) if want_sums else None
        w = np.zeros((len(ref), passes, n_ms), dtype=np.float64) if want_sums else None
        folds = np.zeros((len(ref), passes), dtype=_lib.WEAK_MEASURE_FOLD) if want_sums else None
        self._check(self.lib.gyp_weak_measure(self.ctx, ptr(iq) if iq.size else None, int(n_streams), int(first_ms), n_ms, ptr(ref) if ref.size else None,
                                               len(ref), ptr(prm), ptr(out), ptr(sums), ptr(w), ptr(folds)))
        return out, sums, w, folds

    def measure_weak_dev(self, iq_ptr: int, n_streams: int, stream_stride: int, first_ms: int, n_ms: int, refined: np.ndarray, out_ptr: int,
                         params=None, sums_ptr: int = 0, w_ptr: int = 0, folds_ptr: int = 0) -> None:
        """Device-pointer form: waits for the stream once, after uploading the candidates, then only enqueues."""
        ref = np.ascontiguousarray(refined, dtype=_lib.WEAK_REFINED).reshape(-1)
        self._check(self.lib.gyp_weak_measure_dev(self.ctx, C.c_void_p(iq_ptr or None), int(n_streams), int(stream_stride), int(first_ms), int(n_ms),
                                                   ptr(ref) if ref.size else None, len(ref), ptr(_measure_params(params)), C.c_void_p(out_ptr or None),
                                                   C.c_void_p(sums_ptr or None), C.c_void_p(w_ptr or None), C.c_void_p(folds_ptr or None)))

    def synth_iq(self, out: "DeviceBuffer", n_streams: int, stream_stride: int, n_ms: int, sats: np.ndarray,
                 noise_sigma: float, seed: int) -> None:
        """Generate synthetic baseband straight into HBM (bench / test support). sats: SYNTH_SAT[n_streams, n_sats]."""
        sats = np.ascontiguousarray(sats, dtype=SYNTH_SAT).reshape(n_streams, -1)
        self._check(self.lib.gyp_synth_iq_dev(self.ctx, out.ptr, n_streams, stream_stride, n_ms, ptr(sats),
                                               sats.shape[1], float(noise_sigma), int(seed)))

    def synth_nav_bit(self, seed: int, stream: int, sat_id: int, offset_ms: int, ms: int) -> int:
        return int(self.lib.gyp_synth_nav_bit(int(seed), stream, sat_id, offset_ms, ms))

    # ------------------------------------------------------------------ tracking
    def track_step(self, iq_1ms: np.ndarray, n_streams: int, start_times: Sequence[float], chans: np.ndarray,
                   want_profiles: bool = False) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        iq = _iq_arg(iq_1ms, (n_streams, self.n))
        t0 = np.ascontiguousarray(start_times, dtype=np.float64)
        chans = np.ascontiguousarray(chans, dtype=CHAN_IN)
        out = np.zeros(len(chans), dtype=CHAN_OUT)
        prof = np.zeros((len(chans), self.n), dtype=np.float32) if want_profiles else None
        self._check(self.lib.gyp_track_step(self.ctx, ptr(iq), n_streams, ptr(t0), ptr(chans), len(chans), ptr(out),
                                             ptr(prof)))
        return out, prof

    def create_bank(self, inits: np.ndarray) -> "ChannelBank":
        return ChannelBank(self, inits)

    def create_weak_bank(self, inits: np.ndarray, params=None, first_ms: int = 0) -> "WeakChannelBank":
        """A weak bank (gyp_weak_bank_*): CHAN_INIT records (or WEAK_RESULT fields copied into them), a _records.WeakParams or a
        WEAK_PARAMS record (None: the defaults), the absolute index of the first millisecond it will be given."""
        return WeakChannelBank(self, inits, params, first_ms)


def weak_params_default() -> np.ndarray:
    """gyp_weak_params_default (host only, no GPU): one WEAK_PARAMS record."""
    rec = np.zeros(1, dtype=_lib.WEAK_PARAMS)
    _lib.load().gyp_weak_params_default(ptr(rec))
    return rec


def weak_bit_sync(prompts: np.ndarray, first_ms: int) -> Tuple[np.ndarray, int]:
    """gyp_weak_bit_sync (host only, no GPU): (energies float64[20], edge offset) of the complex64 prompts of milliseconds
    first_ms, first_ms + 1, ..."""
    lib = _lib.load()
    p = np.ascontiguousarray(prompts, dtype=np.complex64).reshape(-1)
    en = np.zeros(20, dtype=np.float64)
    off = np.zeros(1, dtype=np.int32)
    rc = lib.gyp_weak_bit_sync(ptr(p) if p.size else None, p.size, int(first_ms), ptr(en), ptr(off))
    if rc != 0:
        raise GypsumHipError(rc, (lib.gyp_last_error(None) or b"").decode())
    return en, int(off[0])


def _refine_params(params) -> Optional[np.ndarray]:
    """A _records.WeakRefineParams or a WEAK_REFINE_PARAMS record as the library takes it (None stays None: the defaults)."""
    if params is not None and not isinstance(params, np.ndarray):
        params = params.record()
    return None if params is None else np.ascontiguousarray(params, dtype=_lib.WEAK_REFINE_PARAMS).reshape(-1)


def weak_refine_params_default() -> np.ndarray:
    """gyp_weak_refine_params_default (host only, no GPU): one WEAK_REFINE_PARAMS record."""
    rec = np.zeros(1, dtype=_lib.WEAK_REFINE_PARAMS)
    _lib.load().gyp_weak_refine_params_default(ptr(rec))
    return rec


def weak_refine_estimate(prompts: np.ndarray, first_ms: int, params=None) -> np.ndarray:
    """gyp_weak_refine_estimate (host only, no GPU): one WEAK_REFINED record from the complex64 prompts of milliseconds first_ms,
    first_ms + 1, ...: the residual Doppler (delta_hz; the input Doppler and carrier phase count as 0), the carrier-phase increment,
    the bit edge and the quality figures."""
    lib = _lib.load()
    p = np.ascontiguousarray(prompts, dtype=np.complex64).reshape(-1)
    out = np.zeros(1, dtype=_lib.WEAK_REFINED)
    rc = lib.gyp_weak_refine_estimate(ptr(p) if p.size else None, p.size, int(first_ms), ptr(_refine_params(params)), ptr(out))
    if rc != 0:
        raise GypsumHipError(rc, (lib.gyp_last_error(None) or b"").decode())
    return out[0]


def _measure_params(params) -> Optional[np.ndarray]:
    """A _records.WeakMeasureParams or a WEAK_MEASURE_PARAMS record as the library takes it (None stays None: the defaults)."""
    if params is not None and not isinstance(params, np.ndarray):
        params = params.record()
    return None if params is None else np.ascontiguousarray(params, dtype=_lib.WEAK_MEASURE_PARAMS).reshape(-1)


def weak_measure_params_default() -> np.ndarray:
    """gyp_weak_measure_params_default (host only, no GPU): one WEAK_MEASURE_PARAMS record."""
    rec = np.zeros(1, dtype=_lib.WEAK_MEASURE_PARAMS)
    _lib.load().gyp_weak_measure_params_default(ptr(rec))
    return rec


def weak_measure_estimate(sums: np.ndarray, w: np.ndarray, first_ms: int, edge: int, c0: int, spacing: int = 1 << 39) -> np.ndarray:
    """gyp_weak_measure_estimate (host only, no GPU): one WEAK_MEASURE_FOLD record -- the envelopes' energies over the data bits at
    `edge`, the noise share, the correction dd, the corrected c0 and the C/N0 -- from one pass's WEAK_MS_REC sums and float64 W_m of
    milliseconds first_ms, first_ms + 1, ... and the pass's c0."""
    lib = _lib.load()
    s = np.ascontiguousarray(sums, dtype=_lib.WEAK_MS_REC).reshape(-1)
    ww = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
    if len(s) != len(ww):
        raise ValueError("one W per millisecond record expected")
    out = np.zeros(1, dtype=_lib.WEAK_MEASURE_FOLD)
    rc = lib.gyp_weak_measure_estimate(ptr(s) if s.size else None, ptr(ww) if ww.size else None, len(s), int(first_ms), int(edge), int(spacing), int(c0), ptr(out))
    if rc != 0:
        raise GypsumHipError(rc, (lib.gyp_last_error(None) or b"").decode())
    return out[0]


def weak_measured_state(measured, fs: int, samples_per_ms: int, ms_ahead: int = 0) -> np.ndarray:
    """gyp_weak_measured_state (host only, no GPU): the WEAK_STATE record WeakChannelBank.set_state takes, from one WEAK_MEASURED record,
    advanced ms_ahead milliseconds open loop (0: a bank whose cursor is the buffer's first millisecond; n_ms: one that continues behind it)."""
    lib = _lib.load()
    rec = np.ascontiguousarray(measured, dtype=_lib.WEAK_MEASURED).reshape(-1)[:1]
    out = np.zeros(1, dtype=_lib.WEAK_STATE)
    rc = lib.gyp_weak_measured_state(ptr(rec), int(fs), int(samples_per_ms), int(ms_ahead), ptr(out))
    if rc != 0:
        raise GypsumHipError(rc, (lib.gyp_last_error(None) or b"").decode())
    return out[0]


class _BankHandle:
    """What the two kinds of bank share: the engine, the handle from `create(byref(handle))` and its destruction, the channel count and
    the slot calls.  `_prefix` names the kind's entry points."""
    _prefix = ""

    def __init__(self, engine: "GypsumEngine", n_chan: int, create) -> None:
        self.engine = engine
        self.handle = None             # (a refused create raises below: close() must find the attribute)
        h = C.c_void_p()
        engine._check(create(C.byref(h)))
        self.handle = h
        self.n_chan = n_chan

    def _entry(self, name: str):
        return getattr(self.engine.lib, self._prefix + name)

    def close(self) -> None:
        if self.handle:
            self._entry("destroy")(self.handle)
            self.handle = None

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass

    def set_channel(self, index: int, init) -> None:
        """(Re)start one slot from an acquisition result: fresh loop state and histories (a weak bank's slot in SYNC at the cursor)."""
        one = np.zeros(1, dtype=CHAN_INIT)
        one[0] = init
        self.engine._check(self._entry("set_channel")(self.handle, int(index), ptr(one)))

    def drop_channel(self, index: int) -> None:
        self.engine._check(self._entry("drop_channel")(self.handle, int(index)))


class WeakChannelBank(_BankHandle):
    """Device-resident weak-signal channels (gyp_weak_bank_*): 20-ms coherent loops behind an on-device bit synchronisation."""
    _prefix = "gyp_weak_bank_"

    def __init__(self, engine: "GypsumEngine", inits: np.ndarray, params=None, first_ms: int = 0) -> None:
        inits = np.ascontiguousarray(inits, dtype=CHAN_INIT).reshape(-1)
        if params is not None and not isinstance(params, np.ndarray):
            params = params.record()
        prm = None if params is None else np.ascontiguousarray(params, dtype=_lib.WEAK_PARAMS).reshape(-1)
        super().__init__(engine, len(inits), lambda out: engine.lib.gyp_weak_bank_create(engine.ctx, ptr(inits) if inits.size else None, len(inits), ptr(prm),
                                                                                            int(first_ms), out))

    @staticmethod
    def max_periods(n_ms: int) -> int:
        return n_ms // 20 + 1

    def track_block(self, iq: np.ndarray, n_streams: int, first_ms: int, n_ms: int, want_ms: bool = True,
                    want_periods: bool = True) -> Tuple[Optional[np.ndarray], Optional[list]]:
        """Advance n_ms milliseconds from the cursor (first_ms must be it).  (WEAK_MS_REC[n_chan, n_ms] or None, a list with each
        channel's completed WEAK_PERIOD_REC records or None)."""
        e = self.engine
        iq = _iq_arg(iq, (n_streams, n_ms, e.n), check=n_ms >= 1)
        ms = np.zeros((self.n_chan, max(n_ms, 0)), dtype=_lib.WEAK_MS_REC) if want_ms else None
        per = np.zeros((self.n_chan, self.max_periods(max(n_ms, 0))), dtype=_lib.WEAK_PERIOD_REC) if want_periods else None
        cnt = np.zeros(self.n_chan, dtype=np.int32)
        e._check(e.lib.gyp_weak_track_block(self.handle, ptr(iq) if iq.size else None, int(n_streams), int(first_ms), int(n_ms), ptr(ms), ptr(per), ptr(cnt)))
        return ms, ([per[c, :cnt[c]].copy() for c in range(self.n_chan)] if want_periods else None)

    def track_block_dev(self, iq_ptr: int, stream_stride: int, first_ms: int, n_ms: int, ms_ptr: int = 0, period_ptr: int = 0,
                        n_periods_ptr: int = 0) -> None:
        """Device-pointer form: only enqueues on the engine's stream."""
        e = self.engine
        e._check(e.lib.gyp_weak_track_block_dev(self.handle, C.c_void_p(iq_ptr or None), int(stream_stride), int(first_ms), int(n_ms),
                                                C.c_void_p(ms_ptr or None), C.c_void_p(period_ptr or None), C.c_void_p(n_periods_ptr or None)))

    def set_state(self, index: int, f: float, f_int: float, u0: float, c0: int, edge: int) -> None:
        """Put one channel's full loop state; it tracks from the first millisecond m >= cursor with m % 20 == edge."""
        st = np.zeros(1, dtype=_lib.WEAK_STATE)
        st["f"], st["f_int"], st["u0"], st["c0"], st["edge"] = f, f_int, u0, c0, edge
        self.engine._check(self.engine.lib.gyp_weak_bank_set_state(self.handle, int(index), ptr(st)))

    def state(self) -> np.ndarray:
        out = np.zeros(self.n_chan, dtype=_lib.WEAK_STATE)
        self.engine._check(self.engine.lib.gyp_weak_bank_get_state(self.handle, ptr(out), None))
        return out

    @property
    def cursor(self) -> int:
        cur = C.c_int64()
        self.engine._check(self.engine.lib.gyp_weak_bank_get_state(self.handle, None, C.byref(cur)))
        return int(cur.value)


class ChannelBank(_BankHandle):
    """Device-resident tracking channels (gyp_bank_*)."""
    _prefix = "gyp_bank_"

    def __init__(self, engine: GypsumEngine, inits: np.ndarray) -> None:
        inits = np.ascontiguousarray(inits, dtype=CHAN_INIT)
        super().__init__(engine, len(inits), lambda out: engine.lib.gyp_bank_create(engine.ctx, ptr(inits), len(inits), out))

    def track_block(self, iq: np.ndarray, n_streams: int, n_ms: int, start_times: Sequence[float],
                    want_records: bool = True) -> Optional[np.ndarray]:
        e = self.engine
        iq = _iq_arg(iq, (n_streams, n_ms, e.n))
        t0 = np.ascontiguousarray(start_times, dtype=np.float64)
        if len(t0) != n_ms:
            raise ValueError("one start time per millisecond expected")
        rec = np.zeros((self.n_chan, n_ms), dtype=TRACK_REC) if want_records else None
        e._check(e.lib.gyp_track_block(self.handle, ptr(iq), n_streams, n_ms, ptr(t0), ptr(rec)))
        return rec

    def track_block_dev(self, iq_ptr: int, stream_stride: int, n_ms: int, start_times_ptr: int, rec_ptr: int = 0) -> None:
        e = self.engine
        e._check(e.lib.gyp_track_block_dev(self.handle, C.c_void_p(iq_ptr), stream_stride, n_ms,
                                           C.c_void_p(start_times_ptr), C.c_void_p(rec_ptr or None)))

    def quality_dev(self, rec_ptr: int, n_ms: int, window_ms: int, out_ptr: int, bit_offsets=None, chan_stride: Optional[int] = None) -> None:
        """The signal-quality sums of the records track_block_dev left at rec_ptr (n_chan rows of n_ms, or chan_stride apart): one
        gyp_quality_sums per (channel, window) into out_ptr, on the same stream behind the tracking kernels.  Not synchronised."""
        self.engine.track_quality_dev(rec_ptr, self.n_chan, n_ms if chan_stride is None else chan_stride, n_ms, window_ms, out_ptr,
                                      bit_offsets)

    def reset_dev(self, inits_ptr: int) -> None:
        self.engine._check(self.engine.lib.gyp_bank_reset_dev(self.handle, C.c_void_p(inits_ptr)))

    def state(self) -> Dict[str, np.ndarray]:
        f = np.zeros(self.n_chan)
        phi = np.zeros(self.n_chan)
        cp = np.zeros(self.n_chan, dtype=np.int32)
        lost = np.zeros(self.n_chan, dtype=np.int32)
        self.engine._check(self.engine.lib.gyp_bank_get_state(self.handle, ptr(f), ptr(phi), ptr(cp), ptr(lost)))
        return {"doppler_hz": f, "carrier_phase": phi, "code_phase": cp, "lost": lost}

    def keep_profiles(self, depth: int) -> None:
        """Keep the trailing `depth` non-coherent prompt profiles of every channel per block (tracker.py:154,308-309); 0: off."""
        self.engine._check(self.engine.lib.gyp_bank_keep_profiles(self.handle, int(depth)))

    def profiles(self, channel: int) -> np.ndarray:
        """float32[n_rows, N]: the last block's trailing profiles of one channel, oldest first (gyp_bank_read_profiles)."""
        n_rows = np.zeros(1, dtype=np.int32)
        self.engine._check(self.engine.lib.gyp_bank_read_profiles(self.handle, int(channel), None, ptr(n_rows)))
        out = np.zeros((int(n_rows[0]), self.engine.n), dtype=np.float32)
        if out.size:
            self.engine._check(self.engine.lib.gyp_bank_read_profiles(self.handle, int(channel), ptr(out), ptr(n_rows)))
        return out

    def dll_repairs(self) -> np.ndarray:
        """Per channel: milliseconds of the last block in which the exactly re-integrated code loop differed from the
        tracking kernel's provisional one and repaired it (gyp_debug_dll_read); either tracking path counts them."""
        out = np.zeros(self.n_chan, dtype=np.int32)
        self.engine._check(self.engine.lib.gyp_debug_dll_read(self.handle, _lib.ptr(out)))
        return out

    def exact_discriminators(self, n_ms: int) -> np.ndarray:
        """float64[n_chan, n_ms]: the discriminators the exact-sums kernel formed for the last block on the throughput path
        (gyp_debug_disc_read); milliseconds a lost channel did not process read 0."""
        out = np.zeros((self.n_chan, int(n_ms)), dtype=np.float64)
        self.engine._check(self.engine.lib.gyp_debug_disc_read(self.handle, int(n_ms), _lib.ptr(out)))
        return out


_default_engines: Dict[Tuple[int, int, int], GypsumEngine] = {}


def default_engine(samples_per_second: int, samples_per_prn_transmission: int, device: int = 0) -> GypsumEngine:
    """Process-wide engine of one (device, stream format) for the drop-in classes.  One engine per format: a bank or
    tracker created under one sample rate keeps its context when another rate is used next to it."""
    key = (int(device), int(samples_per_second), int(samples_per_prn_transmission))
    eng = _default_engines.get(key)
    if eng is None:
        eng = GypsumEngine(device)
        eng.set_stream_format(samples_per_second, samples_per_prn_transmission)
        _default_engines[key] = eng
    return eng
