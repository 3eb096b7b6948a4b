"""Signal quality of tracked channels: C/N0 and carrier lock (include/gypsum_hip.h, "signal quality").

The device reduces a block's tracking records to sums per (channel, window) -- `engine.track_quality(records, window_ms)` on host
records, `bank.quality_dev(rec_ptr, n_ms, window_ms, out_ptr)` on the records `track_block_dev` left in HBM -- and the host turns
sums into figures:

    sums = engine.track_quality(records, 1000, bit_offsets)      # (n_chan, n_win) QUALITY_SUMS
    q = from_sums(sums)                                          # (n_chan, n_win) QUALITY: cn0_m2m4_dbhz, cn0_nwpr_dbhz, phase_lock, ...

`QualityMonitor` keeps per-channel windows across blocks, so a receiver loop gets the same figures however it cuts its blocks.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

SUMS_DTYPE = _lib.QUALITY_SUMS
QUALITY_DTYPE = _lib.QUALITY
GROUP_MS = 20   # pseudosymbols per navigation bit


def from_sums(sums, combine: bool = False):
    """gyp_quality_from_sums (host only, no GPU).  One QUALITY record per QUALITY_SUMS record of `sums` (same shape; a single
    record gives a single record); with combine=True the records of the last axis are combined into one (consecutive windows of a
    channel).  An estimate that is not defined is NaN."""
    lib = _lib.load()
    s = np.asarray(sums, dtype=SUMS_DTYPE)
    rows = s.reshape(-1, s.shape[-1]) if (combine and s.ndim) else s.reshape(-1, 1)
    out = np.zeros(len(rows), dtype=QUALITY_DTYPE)
    for i, row in enumerate(rows):
        row = np.ascontiguousarray(row)
        rc = lib.gyp_quality_from_sums(_lib.ptr(row), len(row), _lib.ptr(out[i:i + 1]))
        if rc != 0:
            raise _lib.GypsumHipError(rc, (lib.gyp_last_error(None) or b"").decode())
    shape = s.shape[:-1] if (combine and s.ndim) else s.shape
    return out.reshape(shape) if shape else out[0]


def cn0_of_scene(a: float, sigma: float, n: int) -> float:
    """10 log10(1000 a^2 n / (2 sigma^2)) dB-Hz: the C/N0 a single-satellite synthetic scene is built with (amplitude a per sample,
    noise of standard deviation sigma per component, n samples per millisecond)."""
    return float(10.0 * np.log10(1000.0 * a * a * n / (2.0 * sigma * sigma)))


def bit_offset_records(bit_offsets, n_chan: int) -> Optional[np.ndarray]:
    """int32[n_chan] for the library (None stays None: no groups on any channel)."""
    if bit_offsets is None:
        return None
    b = np.ascontiguousarray(bit_offsets, dtype=np.int32).reshape(-1)
    if len(b) != int(n_chan):
        raise ValueError(f"{len(b)} bit offsets for {n_chan} channels")
    return b


class QualityMonitor:
    """Windows of `window_ms` records per channel, counted from the channel's last reset and evaluated as soon as they are complete.

    push(records_block, bit_offsets) takes a block's (n_chan, n_ms) records; bit_offsets[c] is the index, relative to the BLOCK's
    first record, of a record that starts a navigation bit (any such index >= 0: it is reduced mod 20), or None / -1 where the bit
    phase is unknown.  All complete windows of all channels go through ONE gyp_track_quality call.  Returns the new
    (channel, first_record_index, QUALITY record) entries, first_record_index counted from the channel's reset; `last_sums` holds
    their QUALITY_SUMS records in the same order."""

    def __init__(self, engine, n_chan: int, window_ms: int) -> None:
        if int(n_chan) < 1 or int(window_ms) < 1:
            raise ValueError("n_chan and window_ms must be >= 1")
        self.engine = engine
        self.n_chan = int(n_chan)
        self.window_ms = int(window_ms)
        self._pending = [np.zeros(0, dtype=_lib.TRACK_REC) for _ in range(self.n_chan)]   # records of the incomplete window
        self._seen = [0] * self.n_chan                                                    # records since the reset
        self.last_sums = np.zeros(0, dtype=SUMS_DTYPE)

    def seen(self, channel: int) -> int:
        """Records of `channel` pushed since its last reset."""
        return self._seen[int(channel)]

    def reset(self, channel: int = -1) -> None:
        for c in (range(self.n_chan) if channel < 0 else [int(channel)]):
            self._pending[c] = np.zeros(0, dtype=_lib.TRACK_REC)
            self._seen[c] = 0

    def push(self, records_block: np.ndarray, bit_offsets: Optional[Sequence[Optional[int]]] = None) -> List[Tuple[int, int, np.void]]:
        recs = np.asarray(records_block, dtype=_lib.TRACK_REC)
        if recs.ndim != 2 or recs.shape[0] != self.n_chan:
            raise ValueError("records must be (n_chan, n_ms)")
        W = self.window_ms
        rows, offsets, owners = [], [], []
        for c in range(self.n_chan):
            first = self._seen[c] - len(self._pending[c])          # index since the reset of the pending window's first record
            have = np.concatenate([self._pending[c], recs[c]])
            n_win = len(have) // W
            b = None if bit_offsets is None else bit_offsets[c]
            known = b is not None and int(b) >= 0
            for w in range(n_win):
                rows.append(have[w * W:(w + 1) * W])
                # a bit starts at block index b = index len(pending) + b of `have`; relative to this window's first record:
                offsets.append((len(self._pending[c]) + int(b) - w * W) % GROUP_MS if known else -1)
                owners.append((c, first + w * W))
            self._pending[c] = have[n_win * W:].copy()
            self._seen[c] += recs.shape[1]
        if not rows:
            self.last_sums = np.zeros(0, dtype=SUMS_DTYPE)
            return []
        sums = self.engine.track_quality(np.stack(rows), W, np.asarray(offsets, dtype=np.int32)).reshape(-1)
        self.last_sums = sums
        q = from_sums(sums)
        return [(c, first, q[i]) for i, (c, first) in enumerate(owners)]
